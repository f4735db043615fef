"""numpy / Python reference of include/nerf_hip.h "connected components" (a helper module, not a conftest): a sequential
union-find over the lattice edges whose two ends are inside, the smaller root winning, so a root is its component's smallest
linear index.  It calls nothing of the code under test."""
import numpy as np


def inside_mask(vol, iso):
    """bool [R, R, R]: v > iso (NaN and v == iso are outside)."""
    vol = np.asarray(vol)
    assert vol.dtype == np.float32 and vol.ndim == 3 and vol.shape[0] == vol.shape[1] == vol.shape[2]
    with np.errstate(invalid="ignore"):
        return vol > np.float32(iso)


def inside_edges(ins):
    """int64 [E, 2]: the pairs (p, q = p + stride) of linear indices p = i + R (j + R k) of lattice neighbours (+1 along one axis,
    inside the lattice: no wrap) that are both inside."""
    R = ins.shape[0]
    lin = np.arange(R ** 3, dtype=np.int64).reshape(R, R, R)          # [k, j, i]
    out = []
    for axis in (2, 1, 0):                                            # x, y, z
        a = [slice(None)] * 3
        b = [slice(None)] * 3
        a[axis], b[axis] = slice(0, R - 1), slice(1, R)
        both = ins[tuple(a)] & ins[tuple(b)]
        out.append(np.stack([lin[tuple(a)][both], lin[tuple(b)][both]], 1))
    return np.concatenate(out)


def label(vol, iso):
    """int32 [R^3]: -1 at an outside voxel, else the smallest linear index of its 6-connected component."""
    ins = inside_mask(vol, iso)
    parent = list(range(ins.size))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]                             # path halving
            x = parent[x]
        return x

    for p, q in inside_edges(ins).tolist():
        a, b = find(p), find(q)
        if a != b:
            parent[max(a, b)] = min(a, b)
    labels = np.full(ins.size, -1, np.int32)
    for p in np.flatnonzero(ins.reshape(-1)).tolist():
        labels[p] = find(p)
    return labels


def sizes_stats(labels):
    """(sizes int32 [R^3]: the voxel count at each root, 0 elsewhere; stats int64 [3]: components, inside voxels, the label of
    the largest component -- the most voxels, ties to the smaller label -- or -1)."""
    labels = np.asarray(labels).reshape(-1)
    kept = labels[labels >= 0].astype(np.int64)
    sizes = np.bincount(kept, minlength=labels.size).astype(np.int32)
    roots = np.flatnonzero(sizes)
    assert (labels[roots] == roots).all()
    largest = -1
    if len(roots):
        largest = int(roots[np.argmax(sizes[roots])])                 # argmax returns the first maximum: the smaller label
    return sizes, np.array([len(roots), len(kept), largest], np.int64)


def components(vol, iso):
    labels = label(vol, iso)
    sizes, stats = sizes_stats(labels)
    return labels, sizes, stats


def dropped_mask(labels, sizes, stats, min_voxels=0, largest_only=False):
    """bool [R^3]: inside voxels whose component has fewer than min_voxels voxels or, with largest_only, is not the largest."""
    labels = np.asarray(labels).reshape(-1)
    ins = labels >= 0
    drop = np.zeros(labels.size, bool)
    size_of = np.asarray(sizes).reshape(-1)[np.where(ins, labels, 0)].astype(np.int64)
    drop |= ins & (size_of < int(min_voxels))
    if largest_only:
        drop |= ins & (labels != int(stats[2]))
    return drop


def filter_volume(vol, iso, min_voxels=0, largest_only=False, comps=None):
    """float32 [R, R, R]: iso at the dropped voxels, every other value copied bit for bit."""
    vol = np.ascontiguousarray(vol, dtype=np.float32)
    labels, sizes, stats = comps if comps is not None else components(vol, iso)
    drop = dropped_mask(labels, sizes, stats, min_voxels, largest_only)
    bits = vol.reshape(-1).view(np.uint32).copy()
    bits[drop] = np.array([iso], np.float32).view(np.uint32)[0]
    return bits.view(np.float32).reshape(vol.shape)


def kept_vertex_mask(vol, iso, drop):
    """bool [V] over the vertices of marching cubes on `vol` in their order (by owner linear index, then axis x, y, z): the
    crossing edge's inside end is not dropped."""
    ins = inside_mask(vol, iso)
    R = ins.shape[0]
    drop = np.asarray(drop).reshape(R, R, R)
    cross = np.zeros((R, R, R, 3), bool)
    keep = np.zeros((R, R, R, 3), bool)
    for a, axis in enumerate((2, 1, 0)):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, R - 1), slice(1, R)
        lo, hi = tuple(lo), tuple(hi)
        c = ins[lo] != ins[hi]
        cross[lo + (a,)] = c
        keep[lo + (a,)] = c & ~np.where(ins[lo], drop[lo], drop[hi])
    return keep.reshape(-1)[cross.reshape(-1)]
