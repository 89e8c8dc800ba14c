"""Multi-GPU partition of the job space and the film reduce.

Jobs are (tile, wave) pairs keyed by job id; every wave covers the whole image, so sharding by
wave balances perfectly and keeps every RNG stream identical to the 1-GPU / CPU runs.

* ``weak``:  rank r renders its own block of ``spp`` waves, r*spp+1 .. (r+1)*spp — the per-GPU
             work is fixed as N grows and the reduced film holds N*spp samples per pixel.
* ``strong``: the ``spp`` waves of one image are split into N contiguous, balanced blocks (the
             round-robin deal of SURVEY §8e balances the same way; contiguous blocks keep it to one
             persistent-kernel launch per rank), so N GPUs share one fixed image.

* ``bands``: rank r renders all ``spp`` waves of its own band of consecutive tiles, the bands cut for about
             equal estimated cost (``cost_bands``), with one band launch (``Integrator.render_tiles``).  The
             reduced film is bit-identical to the one-GPU film, which the wave shares are not: there the
             all-reduce adds each pixel's partial sums in another fp32 association (equal to ~1e-5 relative
             only).  The argument: every rank's film starts from +0.0; a band launch adds a pixel's samples
             in wave order, the one-GPU order, and touches no pixel outside its band; a film that starts at
             +0.0 never holds -0.0 (x + y is -0.0 only when both are -0.0, and the running sum is not); so
             every pixel is one rank's exact value plus +0.0 from the others, and x + (+0.0) == x exactly,
             in any rank order and any reduction tree.

After rendering, the H*W*4 fp32 films are summed over the ranks with one all-reduce
(RCCL over xGMI for the "nccl" backend; gloo in the CPU tests) — the only exchange the path has.
"""
from __future__ import annotations

from typing import List, Tuple


def rank_wave_ranges(rank: int, world: int, spp: int, mode: str = "weak") -> List[Tuple[int, int]]:
    """Contiguous (first_wave, num_waves) runs this rank renders (waves are 1-based)."""
    if not (0 <= rank < world) or spp <= 0:
        raise ValueError("bad rank/world/spp")
    if mode == "weak":
        return [(1 + rank * spp, spp)]
    if mode == "strong":
        base, extra = divmod(spp, world)
        first = 1 + rank * base + min(rank, extra)
        n = base + (1 if rank < extra else 0)
        return [(first, n)] if n else []
    raise ValueError(f"unknown mode {mode!r}")


def rank_job_ranges(rank: int, world: int, spp: int, jobs_per_wave: int, mode: str = "weak"):
    """The same partition as job-id ranges (jid_begin, jid_count)."""
    return [((w - 1) * jobs_per_wave, n * jobs_per_wave) for w, n in rank_wave_ranges(rank, world, spp, mode)]


def cost_bands(cost, n: int) -> List[int]:
    """n bands of consecutive tiles [cut[i], cut[i + 1]) of about equal estimated cost, each at least one tile:
    the cuts of vpt_gpu::detail::cost_bands (include/vpt_run.hpp), accumulated in float64 over the float32 costs
    (negative ones count as 0).  Raises ValueError when there are fewer tiles than bands."""
    import numpy as np

    c = np.maximum(np.asarray(cost, dtype=np.float32).reshape(-1), np.float32(0.0)).astype(np.float64)
    T, n = int(c.shape[0]), int(n)
    if n < 1 or T < n:
        raise ValueError(f"cost_bands: {T} tiles cannot make {n} non-empty bands")
    total = 0.0
    for v in c.tolist():  # (the same left-to-right float64 sum)
        total += v
    cl = c.tolist()
    cut = [0] * (n + 1)
    acc, t = 0.0, 0
    for i in range(1, n):
        goal = total * float(i) / float(n)
        while t < T and acc + cl[t] <= goal:
            acc += cl[t]
            t += 1
        t = max(t, cut[i - 1] + 1)  # non-empty bands
        t = min(t, T - (n - i))  # room for the rest
        cut[i] = t
    cut[n] = T
    return cut


def rank_tile_band(rank: int, world: int, cost) -> Tuple[int, int]:
    """(tile_lo, tile_hi) of this rank's band of the cost-balanced partition (needs no GPU)."""
    if not (0 <= rank < world):
        raise ValueError("bad rank/world")
    cut = cost_bands(cost, world)
    return cut[rank], cut[rank + 1]


def total_samples_per_pixel(world: int, spp: int, mode: str = "weak") -> int:
    return spp * world if mode == "weak" else spp


def _shared_cuts(cut: List[int], group=None) -> List[int]:
    """Rank 0's cuts on every rank of an initialised process group (cost estimates computed on different devices
    could differ in a last bit, and cuts that disagree would leave gaps or overlaps in the film)."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1):
        return cut
    t = torch.tensor(cut, dtype=torch.int64)
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    dist.broadcast(t, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    return [int(v) for v in t.cpu().tolist()]


def render_rank(integrator, rank: int, world: int, spp: int, mode: str = "weak", film=None, stream=None, group=None):
    """Launch this rank's share of the job space on its integrator (asynchronously, on `stream`) into
    `film` (default: the integrator's own).  Returns the (jid_begin, count) ranges launched; in the ``bands``
    mode the rank's band, [(tile_lo, tile_hi)], cut from the integrator's tile costs (rank 0's cuts on every
    rank of `group` when a process group is initialised)."""
    if mode == "bands":
        if not (0 <= rank < world) or spp <= 0:
            raise ValueError("bad rank/world/spp")
        cost, _ = integrator.tile_costs()
        cut = _shared_cuts(cost_bands(cost, world), group)
        lo, hi = cut[rank], cut[rank + 1]
        integrator.render_tiles(lo, hi, 1, spp, film=film, stream=stream)
        return [(lo, hi)]
    ranges = rank_job_ranges(rank, world, spp, integrator.jobs_per_wave, mode)
    for b, n in ranges:
        integrator.render_jobs(b, n, film=film, stream=stream)
    return ranges


def reduce_film(film, group=None):
    """Sum the per-rank films in place (every rank ends with the whole image): RCCL over xGMI for a
    device film with the "nccl" backend; with gloo (CPU tests, several ranks sharing one GPU) a
    device film is summed through a host copy."""
    import torch.distributed as dist

    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        if film.is_cuda and dist.get_backend(group) == "gloo":
            host = film.cpu()
            dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
            film.copy_(host)
        else:
            dist.all_reduce(film, op=dist.ReduceOp.SUM, group=group)
    return film
