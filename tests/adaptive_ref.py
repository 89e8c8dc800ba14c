"""numpy float32 restatements for the adaptive-sampling tests (include/vpt_gpu.h, "Adaptive sampling"): the moment
plane the ordered film passes keep, the per-tile error estimate with its fixed reduction tree, and the driver's
rule.  Every operation is a separate fp32 numpy operation (no fused multiply-add, correctly rounded division and
square root), in the order the header states, so the GPU's results can be compared bit for bit."""
import numpy as np

F = np.float32


def tile_rect(cfg, t):
    tw, th = int(cfg.tile_size[0]), int(cfg.tile_size[1])
    ntx = -(-cfg.width // tw)
    x0, y0 = (t % ntx) * tw, (t // ntx) * th
    return x0, y0, min(cfg.width - x0, tw), min(cfg.height - y0, th)


def tile_mask(cfg, tiles):
    m = np.zeros((cfg.height, cfg.width), bool)
    for t in tiles:
        x0, y0, rw, rh = tile_rect(cfg, t)
        m[y0:y0 + rh, x0:x0 + rw] = True
    return m


def records_to_samples(cfg, rec, wave_begin, waves):
    """The oracle's per-sample records of the jobs [wave_begin * T, (wave_begin + waves) * T) (oracle_lib.render_jobs
    records=True: L of job j's local pixel q at rec[j * area + q]) as L[waves][H][W][3]; NaN where a pixel has no
    sample (every other pixel in single-pixel mode)."""
    T = cfg.jobs_per_wave()
    area = int(cfg.tile_size[0] * cfg.tile_size[1])
    rec = rec.reshape(waves, T, area, 3)
    L = np.full((waves, cfg.height, cfg.width, 3), np.nan, np.float32)
    for t in range(T):
        x0, y0, rw, rh = tile_rect(cfg, t)
        L[:, y0:y0 + rh, x0:x0 + rw] = rec[:, t, :rw * rh].reshape(waves, rh, rw, 3)
    return L


def accumulate(cfg, L, film=None, m2=None):
    """Adds the samples L[waves][H][W][3] pixel by pixel in wave order: per sample w += 1, xyz += r * L, then
    y = r * L.y, m2 += y * y (sequential fp32).  -> (film, m2) after every wave: lists of waves + 1 states."""
    r = F(cfg.camera_parameters.imaging_ratio)
    film = np.zeros(L.shape[1:3] + (4,), np.float32) if film is None else film.copy()
    m2 = np.zeros(L.shape[1:3], np.float32) if m2 is None else m2.copy()
    films, m2s = [film.copy()], [m2.copy()]
    for w in range(L.shape[0]):
        has = ~np.isnan(L[w, ..., 0])
        s = np.where(has[..., None], L[w], F(0))
        y = r * s[..., 1]
        nf = film.copy()
        nf[..., 3] = film[..., 3] + F(1)
        nf[..., 0] = film[..., 0] + r * s[..., 0]
        nf[..., 1] = film[..., 1] + y
        nf[..., 2] = film[..., 2] + r * s[..., 2]
        nm = m2 + y * y
        film = np.where(has[..., None], nf, film)
        m2 = np.where(has, nm, m2)
        films.append(film.copy())
        m2s.append(m2.copy())
    return films, m2s


def tree_sum(a):
    """The fixed tree: for h = P/2, P/4, .., 1: a[i] = a[i] + a[i + h], i < h (len(a) a power of two)."""
    a = np.array(a, np.float32)
    h = len(a) // 2
    while h >= 1:
        a[:h] = a[:h] + a[h:2 * h]
        h //= 2
    return a[0]


def tile_errors(cfg, film, m2, abs_floor):
    """vpt_gpu_tile_errors restated -> float32[T]."""
    T = cfg.jobs_per_wave()
    area = int(cfg.tile_size[0] * cfg.tile_size[1])
    P = 1
    while P < area:
        P *= 2
    wp = cfg.worker_parameters
    err = np.zeros(T, np.float32)
    floor = F(abs_floor)
    with np.errstate(all="ignore"):
        for t in range(T):
            x0, y0, rw, rh = tile_rect(cfg, t)
            f = film[y0:y0 + rh, x0:x0 + rw].reshape(-1, 4).astype(np.float32)
            m = m2[y0:y0 + rh, x0:x0 + rw].reshape(-1).astype(np.float32)
            n = f[:, 3]
            counted = n >= F(2)
            if wp.single_pixel_enabled:
                ys, xs = np.mgrid[y0:y0 + rh, x0:x0 + rw]
                counted &= ((xs == int(wp.single_pixel_coord[0])) & (ys == int(wp.single_pixel_coord[1]))).reshape(-1)
            mean = f[:, 1] / n
            ex2 = m / n
            v = ex2 - mean * mean
            v = np.where(v > F(0), v, F(0)).astype(np.float32)
            se = np.sqrt(v / (n - F(1)))
            se_p, mean_p = np.zeros(P, np.float32), np.zeros(P, np.float32)
            se_p[:rw * rh] = np.where(counted, se, F(0))
            mean_p[:rw * rh] = np.where(counted, mean, F(0))
            cnt = int(counted.sum())
            if cnt:
                err[t] = tree_sum(se_p) / (tree_sum(mean_p) + floor * F(cnt))
    return err


def emulate_adaptive(cfg, films, m2s, target, abs_floor, min_waves, step_waves, max_waves):
    """The driver's rule on the per-wave states of `accumulate` -> (film, m2, waves uint32[T], err float32[T])."""
    T = cfg.jobs_per_wave()
    waves = np.full(T, min_waves, np.uint32)
    film, m2 = films[min_waves].copy(), m2s[min_waves].copy()
    active = list(range(T))
    done = min_waves
    while True:
        err = tile_errors(cfg, film, m2, abs_floor)
        if done >= max_waves:
            break
        active = [t for t in active if err[t] > F(target) or target == 0]  # (target 0: no tile ever stops)
        if not active:
            break
        done += min(step_waves, max_waves - done)
        m = tile_mask(cfg, active)
        film[m], m2[m] = films[done][m], m2s[done][m]
        waves[active] = done
    return film, m2, waves, err


def hand_made_film(cfg):
    """A film and plane with pixels of 0, 1 and many samples, an all-equal tile and an all-black tile."""
    rng = np.random.default_rng(5)
    H, W = cfg.height, cfg.width
    film = np.zeros((H, W, 4), np.float32)
    n = rng.integers(2, 40, (H, W)).astype(np.float32)
    y = rng.random((H, W, 40), np.float32) * F(3)
    k = np.arange(40)[None, None, :] < n[..., None]
    film[..., 1] = np.where(k, y, 0).astype(np.float32).sum(-1, dtype=np.float32)
    film[..., 0] = film[..., 1] * F(0.5)
    film[..., 2] = film[..., 1] * F(2)
    film[..., 3] = n
    m2 = np.where(k, y * y, 0).astype(np.float32).sum(-1, dtype=np.float32)
    # tile 1: all equal (every sample 0.7: m2 / n - mean^2 cancels to about 0, of either sign)
    x0, y0, rw, rh = tile_rect(cfg, 1)
    film[y0:y0 + rh, x0:x0 + rw, 3] = F(9)
    film[y0:y0 + rh, x0:x0 + rw, 1] = F(9) * F(0.7)
    m2[y0:y0 + rh, x0:x0 + rw] = F(9) * (F(0.7) * F(0.7))
    # tile 2: all black
    x0, y0, rw, rh = tile_rect(cfg, 2)
    film[y0:y0 + rh, x0:x0 + rw, :3] = 0
    m2[y0:y0 + rh, x0:x0 + rw] = 0
    # tile 3: no pixel counted (n = 0 and n = 1); tile 0: a few such pixels
    x0, y0, rw, rh = tile_rect(cfg, 3)
    film[y0:y0 + rh, x0:x0 + rw, 3] = (np.arange(rw * rh).reshape(rh, rw) % 2).astype(np.float32)
    film[0, 0, 3], film[1, 2, 3] = 0, 1
    return film, m2
