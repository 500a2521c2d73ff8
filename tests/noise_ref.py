"""The numpy restatement of aacn::row_noise (csrc/aac_noise.h), shared by the act-path tests.

The exploration noise of agent row ``row`` in a launch with noise epoch ``epoch``:

    h1 = mix64(mix64(mix64(seed) ^ epoch) ^ (2 row)),  h2 = mix64(h1 ^ 0xD1B54A32D192ED03)
    u1 = ((h1 >> 11) + 1) / 2^53  in (0, 1],  u2 = (h2 >> 11) / 2^53
    (z0, z1) = sqrt(-2 ln u1) (cos 2 pi u2, sin 2 pi u2)                       (Box-Muller, float64)
    var = noise_start + (noise_end - noise_start) / (eps_end - 1) (ep - 1)  if ep <= eps_end else noise_end
    with ep = episode[row // N] (1 without an episode array)

``noise64`` gives (z0 var, z1 var) in float64 (the float64 UAM actor adds exactly this);
``noise32`` the same rounded to float32 (the fp32 kernels: schedule ends given as float32 values,
arithmetic in float64, one rounding at the end).  Pure numpy: tests/test_noise_ref_cpu.py pins the
pieces against scalar Python integers.
"""
import numpy as np

M64 = (1 << 64) - 1
TWO_PI = 6.283185307179586


def mix64(x):
    """SplitMix64 finaliser on a numpy uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mix64_int(x):
    """The same function on one Python integer (the scalar form the vector form is pinned to)."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def box_muller(seed, epoch, rows):
    """(z0, z1): the standard-normal pair of hash(seed, epoch, 2 row) for every row, float64 (n, 2)."""
    rows = np.asarray(rows).astype(np.uint64)
    with np.errstate(over="ignore"):
        h1 = mix64(mix64(mix64(np.uint64(seed & M64)) ^ np.uint64(epoch)) ^ (np.uint64(2) * rows))
    h2 = mix64(h1 ^ np.uint64(0xD1B54A32D192ED03))
    u1 = ((h1 >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740992.0)
    u2 = (h2 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    rr = np.sqrt(-2.0 * np.log(u1))
    return np.stack([rr * np.cos(TWO_PI * u2), rr * np.sin(TWO_PI * u2)], 1)


def row_episode(rows, N, episode):
    """episode[row // N] for every row (all ones without an episode array), float64."""
    rows = np.asarray(rows).astype(np.int64)
    if episode is None:
        return np.ones(len(rows), dtype=np.float64)
    return np.asarray(episode)[rows // N].astype(np.float64)


def var_schedule(ep, eps_end, noise_start, noise_end):
    """The linear schedule to ``eps_end``, ``noise_end`` afterwards (float64)."""
    ns, ne = float(noise_start), float(noise_end)
    ep = np.asarray(ep, dtype=np.float64)
    return np.where(ep <= eps_end, ns + (ne - ns) / (eps_end - 1) * (ep - 1), ne)


def noise64(seed, epoch, rows, N, episode, eps_end, noise_start, noise_end):
    """The float64 noise pair of every row of ``rows``: (n, 2)."""
    var = var_schedule(row_episode(rows, N, episode), eps_end, noise_start, noise_end)
    return box_muller(seed, epoch, rows) * var[:, None]


def noise32(seed, epoch, rows, N, episode, eps_end, noise_start, noise_end):
    """The fp32 kernels' noise: the schedule ends as the float32 values the launch receives, the
    float64 pair rounded once to float32."""
    ns, ne = float(np.float32(noise_start)), float(np.float32(noise_end))
    return noise64(seed, epoch, rows, N, episode, eps_end, ns, ne).astype(np.float32)
