"""numpy float32 restatement of the denoiser (include/vpt_gpu.h, "Denoise"; the code is csrc/vpt_denoise.h).  Every
stated operation is a separate fp32 numpy operation (no fused multiply-add, correctly rounded division and square
root) in the stated order, whole planes at a time, so the GPU's and the host build's results can be compared bit for
bit.  Validity is a boolean plane here: nothing depends on how the kernels encode it."""
import numpy as np

F = np.float32
B3 = [F(0.25), F(0.5), F(0.25)]
H5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
DEFAULTS = dict(iterations=4, sigma_l=4.0, rel_floor=1e-3)


def prepare(film, m2):
    """-> (valid bool[H][W], c float32[H][W][3], v float32[H][W]); c and v are meaningless where not valid."""
    film, m2 = np.asarray(film, np.float32), np.asarray(m2, np.float32)
    with np.errstate(all="ignore"):
        n = film[..., 3]
        valid = n >= F(1)
        c = film[..., :3] / n[..., None]
        ex2 = m2 / n
        d = ex2 - c[..., 1] * c[..., 1]
        d = np.where(d > F(0), d, F(0)).astype(np.float32)
        v = np.where(n >= F(2), d / (n - F(1)), c[..., 1] * c[..., 1]).astype(np.float32)
    return valid, c.astype(np.float32), v


def _shift(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` where that is outside the image."""
    H, W = a.shape[:2]
    out = np.full_like(a, fill)
    ys0, ys1 = max(0, -dy), min(H, H - dy)
    xs0, xs1 = max(0, -dx), min(W, W - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = a[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return out


def iterate(valid, c, v, guides, guide_sigma, step, sigma_l, rel_floor):
    """One a-trous iteration -> (c', v'); pixels that are not valid keep their values."""
    sigma_l, rel_floor = F(sigma_l), F(rel_floor)
    zero = np.zeros(v.shape, np.float32)
    with np.errstate(all="ignore"):
        gs, gw = zero.copy(), zero.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                use = _shift(valid, dy, dx, False)
                vq = _shift(v, dy, dx, F(0))
                b = B3[dy + 1] * B3[dx + 1]
                gs = np.where(use, gs + b * vq, gs)
                gw = np.where(use, gw + b, gw)
        gv = gs / gw
        cy = c[..., 1]
        den = (sigma_l * np.sqrt(gv) + rel_floor * cy) + F(1e-20)
        acc = np.zeros(c.shape, np.float32)
        accv, ws = zero.copy(), zero.copy()
        for dy in (-2, -1, 0, 1, 2):
            for dx in (-2, -1, 0, 1, 2):
                use = _shift(valid, step * dy, step * dx, False)
                if not use.any():
                    continue
                cq = _shift(c, step * dy, step * dx, F(0))
                vq = _shift(v, step * dy, step * dx, F(0))
                d = np.abs(cy - cq[..., 1]) / den
                w = (H5[dy + 2] * H5[dx + 2]) / (F(1) + d * d)
                for g, sg in zip(guides, guide_sigma):
                    e = (g - _shift(g, step * dy, step * dx, F(0))) / F(sg)
                    w = w / (F(1) + e * e)
                acc = np.where(use[..., None], acc + w[..., None] * cq, acc)
                accv = np.where(use, accv + (w * w) * vq, accv)
                ws = np.where(use, ws + w, ws)
        c2 = acc / ws[..., None]
        v2 = accv / (ws * ws)
    return (np.where(valid[..., None], c2, c).astype(np.float32), np.where(valid, v2, v).astype(np.float32))


def denoise(film, m2, guides=(), guide_sigma=None, iterations=4, sigma_l=4.0, rel_floor=1e-3):
    """vpt_gpu_denoise restated -> (out film float32[H][W][4], var float32[H][W])."""
    film = np.ascontiguousarray(film, np.float32)
    guides = [np.asarray(g, np.float32) for g in guides]
    if guide_sigma is None:
        guide_sigma = [0.2] * len(guides)
    assert len(guide_sigma) >= len(guides) and 1 <= iterations <= 6
    valid, c, v = prepare(film, m2)
    for i in range(iterations):
        c, v = iterate(valid, c, v, guides, guide_sigma, 1 << i, sigma_l, rel_floor)
    n = film[..., 3]
    with np.errstate(all="ignore"):
        out = np.concatenate([c * n[..., None], n[..., None]], axis=2).astype(np.float32)
    out = np.where(valid[..., None], out, film)
    return np.ascontiguousarray(out, np.float32), np.where(valid, v, F(0)).astype(np.float32)


def rel_rmse_y(film, ref):
    """Relative RMSE of Y / W against a reference film's, over the pixels both have."""
    with np.errstate(all="ignore"):
        a = film[..., 1].astype(np.float64) / film[..., 3]
        b = ref[..., 1].astype(np.float64) / ref[..., 3]
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.sqrt(np.mean((a[ok] - b[ok]) ** 2)) / np.mean(b[ok]))


# The frames of the bit-exact tests (host build and GPU): (width, height, iterations) by id, each run with 0, 1 and 4
# guides.
FRAMES = {
    "37x21-k5": (37, 21, 5),   # step 16 reaches past both edges
    "1x1": (1, 1, 4),          # the smallest image
    "3x70": (3, 70, 4),        # narrower than the 5 taps
    "130x9": (130, 9, 4),      # more than two wavefront-widths
}
GUIDE_COUNTS = (0, 1, 4)
GUIDE_SIGMA = (0.2, 0.05, 1.0, 0.5)


def hand_made_frame(W, H, n_guides=0, seed=5, nan_invalid=True):
    """A film, plane and guides in adaptive_ref.hand_made_film's style: per pixel 2..39 samples of a smooth image with
    an edge, every 7th pixel unrendered (n = 0; NaN in xyz, plane and guides when nan_invalid), every 5th with one
    sample; a 1 x 1 frame holds one rendered pixel."""
    rng = np.random.default_rng(seed)
    n = rng.integers(2, 40, (H, W)).astype(np.float32)
    idx = np.arange(H * W).reshape(H, W)
    if H * W > 1:
        n[idx % 5 == 1] = 1
        n[idx % 7 == 3] = 0
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    base = (F(0.5) + xs / F(max(W, 2)) + F(1.5) * (ys > F(H) / F(2))).astype(np.float32)
    y = base[..., None] * (F(0.25) + F(1.5) * rng.random((H, W, 40), np.float32))
    k = np.arange(40)[None, None, :] < n[..., None]
    film = np.zeros((H, W, 4), np.float32)
    film[..., 1] = np.where(k, y, 0).astype(np.float32).sum(-1, dtype=np.float32)
    film[..., 0] = film[..., 1] * F(0.5)
    film[..., 2] = film[..., 1] * F(2)
    film[..., 3] = n
    m2 = np.where(k, y * y, 0).astype(np.float32).sum(-1, dtype=np.float32)
    guides = [rng.random((H, W), np.float32) if g else (base / base.max()).astype(np.float32) for g in range(n_guides)]
    if nan_invalid:
        bad = n == 0
        film[bad, :3] = np.nan
        m2[bad] = np.nan
        for g in guides:
            g[bad] = np.nan
    return film, m2, guides
