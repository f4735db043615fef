"""Host reference of the volume-rendering kernels (a helper module for the tests, not a conftest; csrc/sampling.hip and
csrc/composite.hip are the product).

Everything is numpy float32 with ONE rounding per operation, in the operation order of the kernels (the library is built with
-ffp-contract=off, `/` and sqrtf are correctly rounded, f32 subnormals are kept):
  lanes      a ray is one wave of 64 lanes; lane l holds the CH consecutive samples k = l CH + c.  CH = ceil(n / 64) in the
             importance sampler, and the next of {1, 2, 3, 4, 8, 16} in the compositing kernels (with_int_up_to)
  prefixes   a lane-serial running sum inside the lane, then the wave scan; the exclusive value is `inclusive - own`, as written
  wave scans `wave_scan_incl`, `wave_rscan_incl`, `wave_sum` of csrc/common.h step by step: lanes without a source add +0.0f
  float64    the importance sampler's weight sum (xor butterfly) and CDF (lane-serial + Hillis-Steele scan) are float64 and
             rounded to float32 where the kernel rounds them

The one operation a host cannot reproduce is expf.  The emulation takes it as the correctly rounded float32 of the float64 exp of
the float32 argument, and carries beside every value a BOUND: how far a device expf that errs by at most E ulp of its result can
move that value.  A bound is float64 and propagated to first order:
  exp        E ulp(y); 0 where the argument is exactly +-0 (expf(+-0) is exactly 1) -- plus y expm1(bound of the argument)
  a + b      e_a + e_b                 a * b   |a| e_b + |b| e_a + e_a e_b             a / b   (e_a + |a/b| e_b) / (|b| - e_b)
  rounding   an operation whose inputs moved rounds another real number: one more ulp of (|result| + bound).  An operation whose
             inputs all have bound 0 has bound 0: it is reproduced bit for bit
so everything the kernels compute without expf (all of sampling, the MSE gradient, compositing where every x and prefix is 0)
has bound 0.  Values are `V` objects (`.v` float32, `.e` float64); plain arrays are promoted with bound 0.
"""
import numpy as np

f32 = np.float32
f64 = np.float64
WAVE = 64
COMPOSITE_CH = (1, 2, 3, 4, 8, 16)
COMPOSITE_CAP = 8192 * 4          # rays per trip of the compositing kernels' grid-stride loop (8192 workgroups of 4 waves)
IMPORTANCE_CAP = 2048 * 4         # ... of the importance kernel
ELEMENTWISE_CAP = 2048 * 256      # elements per trip of sample_coarse / add_noise_z (grid_for(total, 256))
MSE_CAP = 64 * 256                # ... of the MSE kernel (grid_for(count, 256, 64))
U32 = 2.0 ** -24                  # unit roundoff of float32


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u) for float32: the forward-error factor of a length-n sum in any order."""
    return n * U32 / (1.0 - n * U32)


def composite_ch(n):
    ch = -(-n // WAVE)
    return next(c for c in COMPOSITE_CH if ch <= c)


def ulp(x):
    """Spacing of float32 above |x| (float64); the smallest subnormal for 0."""
    x = np.minimum(np.abs(np.asarray(x, f64)), f64(np.finfo(f32).max)).astype(f32)
    return np.spacing(x).astype(f64)


def exp32(a):
    """Correctly rounded float32 exp of a float32 argument (through float64)."""
    with np.errstate(over="ignore", under="ignore"):
        return np.exp(np.asarray(a, f32).astype(f64)).astype(f32)


class V:
    """float32 values `.v` with a float64 bound `.e` on |device value - v|."""
    __slots__ = ("v", "e")
    __array_ufunc__ = None            # numpy scalars and arrays on the left defer to the reflected operators below

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=f32)
        self.e = np.zeros(self.v.shape, f64) if e is None else np.broadcast_to(np.asarray(e, f64), self.v.shape)

    @staticmethod
    def of(x):
        return x if isinstance(x, V) else V(x)

    def _done(self, v, e):
        with np.errstate(all="ignore"):
            e = np.where(e > 0, e + ulp(np.abs(v.astype(f64)) + e), e)        # (a NaN bound stays NaN: nothing is promised)
        return V(v, e)

    def __add__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            return self._done(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            return self._done(self.v - o.v, self.e + o.e)

    def __rsub__(self, o):
        return V.of(o) - self

    def __mul__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            a, b = np.abs(self.v.astype(f64)), np.abs(o.v.astype(f64))
            # (0 * inf = NaN in the bound where a factor is exact and the other infinite: where() keeps exact factors exact)
            e = np.where(o.e > 0, a * o.e, 0.0) + np.where(self.e > 0, b * self.e, 0.0) + self.e * o.e
            return self._done(self.v * o.v, e)

    __radd__ = __add__
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = V.of(o)
        with np.errstate(all="ignore"):
            v = self.v / o.v
            lo = np.abs(o.v.astype(f64)) - o.e
            e = np.where((self.e > 0) | (o.e > 0), np.where(lo > 0, (self.e + np.abs(v.astype(f64)) * o.e) / lo, np.inf), 0.0)
            return self._done(v, e)

    def __rtruediv__(self, o):
        return V.of(o) / self

    def __neg__(self):
        return V(-self.v, self.e)

    def __getitem__(self, i):
        return V(self.v[i], self.e[i])

    def where(self, cond, other):
        o = V.of(other)
        return V(np.where(cond, self.v, o.v), np.where(cond, self.e, o.e))


def vexp(a, E):
    """expf of V `a`: the device errs by at most E ulp of the result."""
    a = V.of(a)
    y = exp32(a.v)
    with np.errstate(all="ignore"):
        own = np.where((a.v == 0) & (a.e == 0), 0.0, E * ulp(y))
        moved = np.where(a.e > 0, y.astype(f64) * np.expm1(a.e), 0.0)
        e = own + moved
        e = np.where(moved > 0, e + ulp(y.astype(f64) + e), e)
    return V(y, e)


def vstack(items, axis=-1):
    return V(np.stack([i.v for i in items], axis), np.stack([i.e for i in items], axis))


# ---- the wave64 scans of csrc/common.h, on [..., 64] -------------------------------------------------------------------------
def _rows(a):
    return a.reshape(a.shape[:-1] + (4, 16))


def _dpp_row_shift(x, o, right):
    """row_shr:o (right) / row_shl:o inside each row of 16; lanes without a source read +0."""
    v, e = _rows(x.v), _rows(x.e)
    sv, se = np.zeros_like(v), np.zeros_like(e)
    if right:
        sv[..., o:], se[..., o:] = v[..., :-o], e[..., :-o]
    else:
        sv[..., :-o], se[..., :-o] = v[..., o:], e[..., o:]
    return V(sv.reshape(x.v.shape), se.reshape(x.e.shape))


def _row_bcast(x, src_lane, rows):
    """row_bcast: lane `src_lane` of the rows below into every lane of `rows`; the other rows read +0."""
    sv, se = np.zeros_like(_rows(x.v)), np.zeros_like(_rows(x.e))
    for r, s in zip(rows, src_lane):
        sv[..., r, :], se[..., r, :] = x.v[..., s, None], x.e[..., s, None]
    return V(sv.reshape(x.v.shape), se.reshape(x.e.shape))


def wave_scan_incl(x):
    x = V.of(x)
    for o in (1, 2, 4, 8):
        x = x + _dpp_row_shift(x, o, True)
    x = x + _row_bcast(x, (15, 47), (1, 3))          # row_bcast:15, row_mask 0xa
    x = x + _row_bcast(x, (31, 31), (2, 3))          # row_bcast:31, row_mask 0xc
    return x


def wave_sum(x):
    return wave_scan_incl(x)[..., 63]


def wave_rscan_incl(x):
    x = V.of(x)
    for o in (1, 2, 4, 8):
        x = x + _dpp_row_shift(x, o, False)
    t1, t2, t3 = x[..., 16], x[..., 32], x[..., 48]
    t23 = t2 + t3
    zero = V(np.zeros_like(t1.v))
    above = vstack([t1 + t23, t23, t3, zero], -1)     # per row
    return x + V(np.repeat(above.v, 16, -1), np.repeat(above.e, 16, -1))


def wave_sum_f64(x):
    """xor butterfly of wave_sum(double): every lane ends with the same value."""
    x = np.asarray(x, f64)
    idx = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., idx ^ o]
    return x[..., 0]


def wave_scan_incl_f64(x):
    x = np.asarray(x, f64).copy()
    for o in (1, 2, 4, 8, 16, 32):
        t = np.zeros_like(x)
        t[..., o:] = x[..., :-o]
        x[..., o:] = x[..., o:] + t[..., o:]
    return x


# ---- depth sampling ----------------------------------------------------------------------------------------------------------
def sample_coarse(near, far, n, lindisp=False, perturb=0.0, t_rand=None):
    """[B, n] float32 coarse depths of per-ray near / far [B] (sample_coarse_kernel)."""
    near = np.asarray(near, f32).reshape(-1, 1)
    far = np.asarray(far, f32).reshape(-1, 1)
    step = f32(1.0 / float(n - 1))
    one = f32(1.0)

    def zk(kk):
        tv = kk.astype(f32) * step + f32(0.0)
        with np.errstate(all="ignore"):
            if not lindisp:
                return near * (one - tv) + far * tv
            return one / (one / (near * (one - tv)) + one / (far * tv))

    k = np.arange(n)[None, :]
    v = zk(k)
    if perturb > 0.0:
        with np.errstate(all="ignore"):
            half = f32(0.5)
            lo = np.where(k == 0, v, half * (zk(np.maximum(k - 1, 0)) + v))
            hi = np.where(k == n - 1, v, half * (v + zk(np.minimum(k + 1, n - 1))))
            v = lo + (hi - lo) * (np.asarray(t_rand, f32).reshape(-1, n) * f32(perturb))
    return v.astype(f32)


def add_noise_z(z, t_rand, strength):
    """Stratified jitter on given depths [B, n] (add_noise_z_kernel)."""
    z = np.asarray(z, f32)
    n = z.shape[-1]
    half = f32(0.5)
    with np.errstate(all="ignore"):
        lo, hi = z.copy(), z.copy()
        if n > 1:
            mids = half * (z[:, :-1] + z[:, 1:])
            lo[:, 1:] = mids
            hi[:, :-1] = mids
        return (lo + (hi - lo) * (np.asarray(t_rand, f32) * f32(strength))).astype(f32)


# ---- importance sampling -----------------------------------------------------------------------------------------------------
def _lane_major(a, ch, fill=0):
    """[B, n] -> [B, 64, ch] (sample k = lane ch + c), padded with `fill`."""
    B, n = a.shape
    out = np.full((B, WAVE * ch), fill, a.dtype)
    out[:, :n] = a
    return out.reshape(B, WAVE, ch)


def merge_rule(z, z_new):
    """THE merge rule: the exact multiset of coarse and new depths, ascending, ties coarse-first (then by position), NaN last."""
    allz = np.concatenate([np.asarray(z, f32), np.asarray(z_new, f32)], -1)
    order = np.argsort(allz, axis=-1, kind="stable")          # numpy sorts NaN last; stable keeps coarse ahead of equal new
    return np.take_along_axis(allz, order, -1)


def importance(z, w, u, eps=1e-5):
    """cdf [B, n+1], inds [B, N] int64, z_new [B, N], z_merged [B, n+N] of importance_kernel (all bound 0)."""
    z, w, u = np.asarray(z, f32), np.asarray(w, f32), np.asarray(u, f32)
    B, n = z.shape
    N = u.shape[1]
    ch = -(-n // WAVE)
    eps = f32(eps)
    with np.errstate(all="ignore"):
        valid = _lane_major(np.ones((B, n), bool), ch, False)
        wl = np.where(valid, _lane_major(w, ch) + f32(0.01), f32(0.0))
        part = np.zeros((B, WAVE), f64)
        for c in range(ch):
            part = part + wl[:, :, c].astype(f64)
        s = wave_sum_f64(part).astype(f32)
        pad = np.fmax(eps - s, f32(0.0))
        padw = pad / f32(n)
        s = s + pad
        run = np.zeros((B, WAVE), f64)
        loc = np.zeros((B, WAVE, ch), f64)
        for c in range(ch):
            pdf = np.where(valid[:, :, c], (wl[:, :, c] + padw[:, None]) / s[:, None], f32(0.0))
            run = run + pdf.astype(f64)
            loc[:, :, c] = run
        incl = wave_scan_incl_f64(run)
        excl = incl - run
        cdf = np.zeros((B, n + 1), f32)
        cdf[:, 1:] = np.fmin(f32(1.0), (excl[:, :, None] + loc).astype(f32)).reshape(B, -1)[:, :n]
        a = np.clip(np.arange(n + 1) - 1, 0, n - 2)
        zmid = (z[:, a + 1] + z[:, a]) / f32(2.0)
        # binary search, as written (a CDF with NaN is not monotone: the path matters)
        unan = np.isnan(u)
        lo = np.zeros((B, N), np.int64)
        hi = np.full((B, N), n + 1, np.int64)
        while True:
            act = lo < hi
            if not act.any():
                break
            mid = (lo + hi) >> 1
            cm = np.take_along_axis(cdf, np.minimum(mid, n), 1)
            right = unan | (cm <= u)
            lo = np.where(act & right, mid + 1, lo)
            hi = np.where(act & ~right, mid, hi)
        inds = lo
        below = np.clip(inds - 1, 0, n)
        above = np.minimum(inds, n)
        cf, ct = np.take_along_axis(cdf, below, 1), np.take_along_axis(cdf, above, 1)
        zf, zt = np.take_along_axis(zmid, below, 1), np.take_along_axis(zmid, above, 1)
        den = ct - cf
        den = np.where(den < eps, f32(1.0), den)
        t = (u - cf) / den
        t = np.where(np.isnan(t), f32(0.0), t)
        t = np.fmin(np.fmax(t, f32(0.0)), f32(1.0))
        z_new = (zf + t * (zt - zf)).astype(f32)
    return cdf, inds, z_new, merge_rule(z, z_new)


# ---- alpha compositing -------------------------------------------------------------------------------------------------------
class _Lane:
    pass


def _composite_lane(raw, z, d, noise, raw_noise_std, E):
    """composite_lane<CH> for every ray: arrays [B, 64, CH]."""
    raw, z, d = np.asarray(raw, f32), np.asarray(z, f32), np.asarray(d, f32)
    B, n = z.shape
    ch = composite_ch(n)
    q = _Lane()
    with np.errstate(all="ignore"):
        q.dnorm = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(f32)
        sigma = raw[..., 3]
        if raw_noise_std > 0.0:
            sigma = sigma + np.asarray(noise, f32) * f32(raw_noise_std)
        dz = np.full((B, n), f32(1e10), f32)
        dz[:, :-1] = z[:, 1:] - z[:, :-1]
        delta = dz * q.dnorm[:, None]
        x = delta * sigma
        q.n, q.ch, q.B = n, ch, B
        q.valid = _lane_major(np.ones((B, n), bool), ch, False)
        q.r, q.g, q.b = (_lane_major(raw[..., i], ch) for i in range(3))
        q.z, q.delta, q.x = _lane_major(z, ch), _lane_major(delta, ch), _lane_major(x, ch)
        summed = _lane_major(np.broadcast_to(np.arange(n) < n - 1, (B, n)), ch, False)      # cumsum runs over x[:-1]
        e1 = vexp(-np.fmax(q.x, f32(0.0)), E)                   # fmaxf: a NaN x gives 0
        alpha = (f32(1.0) - e1).where(q.valid, f32(0.0))
        run = np.zeros((B, WAVE), f32)
        pre = np.zeros((B, WAVE, ch), f32)
        for c in range(ch):
            pre[:, :, c] = run
            run = run + np.where(summed[:, :, c], q.x[:, :, c], f32(0.0))
        incl = wave_scan_incl(run).v
        base = incl - run
        q.T = vexp(-(base[:, :, None] + pre), E)
        q.alpha = alpha
        q.w = (alpha * q.T).where(q.valid, f32(0.0))
    return q


def _unlane(x, n):
    return V(x.v.reshape(x.v.shape[0], -1)[:, :n], x.e.reshape(x.e.shape[0], -1)[:, :n])


def _lane_sum(terms):
    """sr = 0; sr += term_c for c in order; then wave_sum."""
    acc = V(np.zeros(terms.v.shape[:2], f32))
    for c in range(terms.v.shape[2]):
        acc = acc + terms[:, :, c]
    return wave_sum(acc)


def composite_forward(raw, z, d, white=False, noise=None, raw_noise_std=0.0, E=1.0):
    """(rgb [B, 3], disp [B], acc [B], weights [B, n], depth [B]) of composite_fwd_kernel as V (value, bound)."""
    q = _composite_lane(raw, z, d, noise, raw_noise_std, E)
    with np.errstate(all="ignore"):
        sr, sg, sb = _lane_sum(q.w * q.r), _lane_sum(q.w * q.g), _lane_sum(q.w * q.b)
        sd, sa = _lane_sum(q.w * q.z), _lane_sum(q.w)
        if white:
            sr, sg, sb = sr + (f32(1.0) - sa), sg + (f32(1.0) - sa), sb + (f32(1.0) - sa)
        qq = sd / sa
        # fmaxf(1e-10f, q), NaN kept: 1-Lipschitz and unrounded, the bound passes through
        m = V(np.where(np.isnan(qq.v), qq.v, np.fmax(f32(1e-10), qq.v)), qq.e)
        disp = f32(1.0) / m
    return vstack([sr, sg, sb], -1), disp, sa, _unlane(q.w, q.n), sd


def _backward_core(q, gr, gg, gb, gacc, gdep, E):
    """d_raw [B, n, 4] from the lane quantities and the per-ray upstream gradients (V or arrays [B])."""
    ex = lambda a: V.of(a)[:, None, None]
    gr, gg, gb, gacc, gdep = ex(gr), ex(gg), ex(gb), ex(gacc), ex(gdep)
    with np.errstate(all="ignore"):
        G = gr * q.r + gg * q.g + gb * q.b + gacc + gdep * q.z
        Gw = G * q.w
        run = V(np.zeros((q.B, WAVE), f32))
        gw = [None] * q.ch
        for c in range(q.ch - 1, -1, -1):
            gw[c] = run
            run = run + Gw[:, :, c]
        incl = wave_rscan_incl(run)
        after = incl - run
        k = (np.arange(WAVE)[:, None] * q.ch + np.arange(q.ch)[None, :])[None]
        suffix = (after[:, :, None] + vstack(gw, -1)).where(k < q.n - 1, f32(0.0))
        da = (G * q.T * vexp(-q.x, E)).where(q.x > 0, f32(0.0))
        dx = da - suffix
        out = vstack([q.w * gr, q.w * gg, q.w * gb, V(q.delta) * dx], -1)          # [B, 64, CH, 4]
    return V(out.v.reshape(q.B, -1, 4)[:, :q.n], out.e.reshape(q.B, -1, 4)[:, :q.n])


def composite_backward(raw, z, d, d_rgb, d_acc=None, d_depth=None, white=False, noise=None, raw_noise_std=0.0, E=1.0):
    """d_raw [B, n, 4] of composite_bwd_kernel as V."""
    q = _composite_lane(raw, z, d, noise, raw_noise_std, E)
    d_rgb = np.asarray(d_rgb, f32)
    gr, gg, gb = d_rgb[:, 0], d_rgb[:, 1], d_rgb[:, 2]
    zero = np.zeros(q.B, f32)
    with np.errstate(all="ignore"):
        gacc = (zero if d_acc is None else np.asarray(d_acc, f32)) - ((gr + gg) + gb if white else zero)
    gdep = zero if d_depth is None else np.asarray(d_depth, f32)
    return _backward_core(q, gr, gg, gb, gacc, gdep, E)


def _blocks_sum(per_ray_sq, B, cap_blocks, inv):
    """The loss of the fused kernel: per wave the squares of its rays in trip order, per workgroup ((p0 + p1) + p2) + p3, times inv,
    then the workgroups in index order (the device adds them atomically in any order).  Returns (loss V, sum of |addends|)."""
    nblk = min(-(-B // 4), cap_blocks)
    sq = V(np.zeros((nblk, 4), f32))
    trips = -(-B // (nblk * 4))
    sqv, sqe = np.zeros((trips * nblk * 4, 3), f32), np.zeros((trips * nblk * 4, 3), f64)
    sqv[:B], sqe[:B] = per_ray_sq.v, per_ray_sq.e
    live = (np.arange(trips * nblk * 4) < B).reshape(trips, nblk, 4)
    sqv, sqe = sqv.reshape(trips, nblk, 4, 3), sqe.reshape(trips, nblk, 4, 3)
    for t in range(trips):
        for c in range(3):
            sq = (sq + V(sqv[t, :, :, c], sqe[t, :, :, c])).where(live[t], sq)
    blk = (((sq[:, 0] + sq[:, 1]) + sq[:, 2]) + sq[:, 3]) * inv
    tot = V(np.zeros((), f32))
    for b in range(nblk):
        tot = tot + blk[b]
    return tot, float(np.abs(blk.v.astype(f64)).sum())


def composite_mse_backward(raw, z, d, target, white=False, grad_scale=1.0, E=1.0):
    """(rgb [B, 3] V, d_raw [B, n, 4] V, loss V, sum of the |per-workgroup loss addends|) of composite_train_kernel."""
    q = _composite_lane(raw, z, d, None, 0.0, E)
    target = np.asarray(target, f32)
    with np.errstate(all="ignore"):
        inv = f32(1.0) / f32(q.B * 3)
        sr, sg, sb, sa = _lane_sum(q.w * q.r), _lane_sum(q.w * q.g), _lane_sum(q.w * q.b), _lane_sum(q.w)
        if white:
            sr, sg, sb = sr + (f32(1.0) - sa), sg + (f32(1.0) - sa), sb + (f32(1.0) - sa)
        er, eg, eb = sr - target[:, 0], sg - target[:, 1], sb - target[:, 2]
        loss, mag = _blocks_sum(vstack([er * er, eg * eg, eb * eb], -1), q.B, 8192, inv)
        s2 = f32(grad_scale) * f32(2.0)
        gr, gg, gb = s2 * er * inv, s2 * eg * inv, s2 * eb * inv
        gacc = f32(0.0) - ((gr + gg) + gb if white else V(np.zeros(q.B, f32)))
        d_raw = _backward_core(q, gr, gg, gb, gacc, np.zeros(q.B, f32), E)
    return vstack([sr, sg, sb], -1), d_raw, loss, mag


def mse_loss_grad(p, t, grad_scale=1.0):
    """(loss float32, d_pred float32 [count], sum of the |per-workgroup addends|) of mse_kernel.  The gradient is exact; the
    device adds the workgroups' loss terms atomically in any order."""
    p, t = np.asarray(p, f32).reshape(-1), np.asarray(t, f32).reshape(-1)
    count = p.size
    inv = f32(1.0) / f32(count)
    d = p - t
    grad = f32(grad_scale) * f32(2.0) * d * inv
    nblk = min(-(-count // 256), 64)
    stride = nblk * 256
    trips = -(-count // stride)
    dd = np.zeros(trips * stride, f32)
    dd[:count] = d * d
    s = np.zeros(stride, f32)
    for tr in range(trips):
        s = s + dd[tr * stride:(tr + 1) * stride]              # (idle threads add +0: s is never -0)
    wave = wave_sum(s.reshape(nblk, 4, WAVE)).v                # [nblk, 4]
    blk = (((wave[:, 0] + wave[:, 1]) + wave[:, 2]) + wave[:, 3]) * inv
    loss = f32(0.0)
    for b in range(nblk):
        loss = f32(loss + blk[b])
    return loss, grad.astype(f32), float(np.abs(blk.astype(f64)).sum())


# ---- transcription of the two merge branches of importance_kernel (host only; shows which slots each branch writes) ----------
def merge_transcribed(z, z_new, nan_check=True):
    """One ray.  Returns (z_merged as a list with None in the slots nobody wrote, branch name).  `nan_check=False` is the kernel
    before the fix: the ascending branch is taken whatever the new depths hold."""
    z, z_new = [f32(v) for v in z], [f32(v) for v in z_new]
    n, N = len(z), len(z_new)
    P = 2
    while P < N:
        P <<= 1
    out = [None] * (n + N)
    asc = all(z[i] <= z[i + 1] for i in range(n - 1))
    if nan_check:
        asc = asc and not any(v != v for v in z_new)
    if asc:
        s_new = z_new + [f32(np.inf)] * (P - N)
        k = 2
        while k <= P:
            j = k >> 1
            while j > 0:
                for pi in range(P >> 1):
                    i = ((pi & ~(j - 1)) << 1) | (pi & (j - 1))
                    q = i | j
                    a, b = s_new[i], s_new[q]
                    if (a > b) == ((i & k) == 0):
                        s_new[i], s_new[q] = b, a
                j >>= 1
            k <<= 1
        for i in range(n):
            lo, hi = 0, N
            while lo < hi:
                mid = (lo + hi) >> 1
                if s_new[mid] < z[i]:
                    lo = mid + 1
                else:
                    hi = mid
            out[i + lo] = z[i]
        for j in range(N):
            lo, hi = 0, n
            while lo < hi:
                mid = (lo + hi) >> 1
                if z[mid] <= s_new[j]:
                    lo = mid + 1
                else:
                    hi = mid
            out[j + lo] = s_new[j]
        return out, "ascending"
    s_all = z + z_new
    for i, v in enumerate(s_all):
        rank = 0
        for kk, o in enumerate(s_all):
            less = (o < v) or (v != v and o == o) or ((o == v or (o != o and v != v)) and kk < i)
            rank += 1 if less else 0
        out[rank] = v
    return out, "general"
