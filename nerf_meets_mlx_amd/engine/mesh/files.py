"""Mesh files: `write_ply` writes a binary little-endian PLY; `write_obj` an OBJ with its .mtl and the atlas as a .png, which a PLY
cannot carry; `read_ply`, `read_obj` and the PNG pair `png_bytes` / `png_array` read back what they write."""
import os
import struct
import zlib

import numpy as np
import torch

from ._base import Mesh
from .texture import Texture, _check_texture


def write_ply(path: str, mesh: Mesh) -> str:
    """Binary little-endian PLY: vertex x y z nx ny nz (float) [+ red green blue (uchar, round(255 c))], face
    `list uchar int vertex_indices`.  Written under a temporary name, then renamed."""
    v = mesh.verts.detach().cpu().numpy().astype("<f4")
    n = mesh.normals.detach().cpu().numpy().astype("<f4")
    f = mesh.faces.detach().cpu().numpy().astype("<i4")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if mesh.colors is not None:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vert = np.empty(len(v), dtype=fields)
    for k, name in enumerate("xyz"):
        vert[name] = v[:, k]
        vert["n" + name] = n[:, k]
    if mesh.colors is not None:
        c = np.clip(np.nan_to_num(mesh.colors.detach().cpu().numpy().astype(np.float64)), 0.0, 1.0)
        rgb = np.round(255.0 * c).astype(np.uint8)
        for k, name in enumerate(("red", "green", "blue")):
            vert[name] = rgb[:, k]
    face = np.empty(len(f), dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"] = 3
    face["i"] = f
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}"]
    head += [f"property {'float' if t == '<f4' else 'uchar'} {name}" for name, t in fields]
    head += [f"element face {len(f)}", "property list uchar int vertex_indices", "end_header"]
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(("\n".join(head) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())
    os.replace(tmp, path)
    return path


def read_ply(path: str) -> Mesh:
    """The inverse of write_ply (CPU tensors); only the layout write_ply produces."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").splitlines()
    if head[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int(head[2].split()[2])
    props = [ln.split() for ln in head if ln.startswith("property ") and "list" not in ln]
    fields = [(p[2], "<f4" if p[1] == "float" else "u1") for p in props]
    nf = int(next(ln for ln in head if ln.startswith("element face")).split()[2])
    vert = np.frombuffer(data, dtype=fields, count=nv, offset=end)
    face = np.frombuffer(data, dtype=[("n", "u1"), ("i", "<i4", (3,))], count=nf, offset=end + vert.nbytes)
    if end + vert.nbytes + face.nbytes != len(data) or not (face["n"] == 3).all():
        raise ValueError(f"{path}: unexpected PLY layout")
    verts = torch.from_numpy(np.stack([vert[k] for k in "xyz"], 1).copy())
    normals = torch.from_numpy(np.stack([vert["n" + k] for k in "xyz"], 1).copy())
    colors = None
    if "red" in vert.dtype.names:
        colors = torch.from_numpy(np.stack([vert[k] for k in ("red", "green", "blue")], 1).astype(np.float32) / 255.0)
    return Mesh(verts, torch.from_numpy(face["i"].copy()), normals, colors)


def _replace_file(path: str, data: bytes):
    tmp = path + ".tmp"
    with open(tmp, "wb") as fh:
        fh.write(data)
    os.replace(tmp, path)


def _png_chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


_PNG_MAGIC = b"\x89PNG\r\n\x1a\n"


def png_bytes(image: np.ndarray) -> bytes:
    """An 8-bit RGB PNG of a uint8 [H, W, 3] array, every row with filter type 0 (zlib and struct alone)."""
    H, W, _ = image.shape
    lines = np.zeros((H, 1 + 3 * W), np.uint8)
    lines[:, 1:] = image.reshape(H, 3 * W)
    return _PNG_MAGIC + _png_chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)) \
        + _png_chunk(b"IDAT", zlib.compress(lines.tobytes(), 6)) + _png_chunk(b"IEND", b"")


def png_array(data: bytes) -> np.ndarray:
    """The inverse of png_bytes: uint8 [H, W, 3]; ValueError for anything but 8-bit RGB with filter type 0 throughout."""
    if data[:8] != _PNG_MAGIC:
        raise ValueError("not a PNG")
    pos, head, idat = 8, None, b""
    while pos < len(data):
        n, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(kind + body):
            raise ValueError("PNG: bad chunk checksum")
        if kind == b"IHDR":
            head = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        pos += 12 + n
    if head is None or head[2:] != (8, 2, 0, 0, 0):
        raise ValueError("PNG: only 8-bit RGB without interlace")
    W, H = head[:2]
    lines = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(H, 1 + 3 * W)
    if lines[:, 0].any():
        raise ValueError("PNG: only filter type 0")
    return lines[:, 1:].reshape(H, W, 3).copy()


def write_obj(path: str, mesh: Mesh, texture: Texture) -> str:
    """Wavefront OBJ with its material and texture: `path` (v, vn, one vt per face corner, `f a/t/a b/t/b c/t/c`, 1-based; floats
    with nine significant digits, which float32 survives), beside it the same name with the suffix .mtl (one material whose
    map_Kd names the image) and with .png (8-bit RGB, png_bytes).  Vertex colours are not written.  Each file is written under
    a temporary name, then renamed."""
    _check_texture("write_obj", texture, mesh)
    stem = os.path.splitext(path)[0]
    v = mesh.verts.detach().cpu().numpy().astype(np.float64)
    n = mesh.normals.detach().cpu().numpy().astype(np.float64)
    f = mesh.faces.detach().cpu().numpy().astype(np.int64) + 1
    uv = texture.uv.detach().cpu().numpy().astype(np.float64).reshape(-1, 2)
    out = [f"# texels {texture.texels}", f"mtllib {os.path.basename(stem)}.mtl", "usemtl atlas"]
    out += ["v %.9g %.9g %.9g" % tuple(r) for r in v]
    out += ["vn %.9g %.9g %.9g" % tuple(r) for r in n]
    out += ["vt %.9g %.9g" % tuple(r) for r in uv]
    out += ["f %d/%d/%d %d/%d/%d %d/%d/%d" % (a, 3 * k + 1, a, b, 3 * k + 2, b, c, 3 * k + 3, c) for k, (a, b, c) in enumerate(f)]
    _replace_file(stem + ".png", png_bytes(texture.image.detach().cpu().numpy()))
    _replace_file(stem + ".mtl", f"newmtl atlas\nKd 1 1 1\nmap_Kd {os.path.basename(stem)}.png\n".encode("ascii"))
    _replace_file(path, ("\n".join(out) + "\n").encode("ascii"))
    return path


def read_obj(path: str):
    """The inverse of write_obj: (Mesh without colours, Texture) as CPU tensors; only the layout write_obj produces."""
    with open(path) as fh:
        lines = [ln.split() for ln in fh]
    if not lines or lines[0][:2] != ["#", "texels"]:
        raise ValueError(f"{path}: not an OBJ of write_obj")
    T = int(lines[0][2])
    by = {k: [w[1:] for w in lines if w and w[0] == k] for k in ("v", "vn", "vt", "f", "mtllib")}
    verts = torch.tensor(np.array(by["v"], np.float64).reshape(-1, 3), dtype=torch.float32)
    normals = torch.tensor(np.array(by["vn"], np.float64).reshape(-1, 3), dtype=torch.float32)
    uv = torch.tensor(np.array(by["vt"], np.float64).reshape(-1, 3, 2), dtype=torch.float32)
    corners = np.array([[c.split("/") for c in w] for w in by["f"]], np.int64).reshape(-1, 3, 3)
    F = len(corners)
    if len(by["mtllib"]) != 1 or uv.shape[0] != F or normals.shape != verts.shape \
            or not np.array_equal(corners[:, :, 1].reshape(-1), np.arange(1, 3 * F + 1)) \
            or not np.array_equal(corners[:, :, 0], corners[:, :, 2]):
        raise ValueError(f"{path}: unexpected OBJ layout")
    here = os.path.dirname(path)
    with open(os.path.join(here, by["mtllib"][0][0])) as fh:
        maps = [ln.split()[1] for ln in fh if ln.startswith("map_Kd ")]
    if len(maps) != 1:
        raise ValueError(f"{path}: the material needs one map_Kd")
    with open(os.path.join(here, maps[0]), "rb") as fh:
        image = torch.from_numpy(png_array(fh.read()))
    faces = torch.from_numpy((corners[:, :, 0] - 1).astype(np.int32))
    return Mesh(verts, faces, normals), Texture(image, uv, T)
