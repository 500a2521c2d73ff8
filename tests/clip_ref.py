"""References for the gradient-clipping tests (TEST INFRASTRUCTURE ONLY).

``ClippedAdam``      torch.optim.Adam whose ``step()`` first calls ``clip_grad_norm_`` on its parameters, as
                     the reference's ``update()`` does before every optimiser step (ATT/maddpg:187,
                     :205-206), and records the returned norm.  The oracle restatements (``ref_update``,
                     ``ref_update_dp``, ``ref_gru_update``) take ``opts``: passing these drives them
                     with clipping, nothing under ``oracle/`` changes.
``sum_copies``       the split-K copies summed in the element type in the Adam kernels' two orders.
``clip_adam``        float64 numpy restatement of aac_clip_sumsq + aac_adam_flat_clip (include/aac_clip.h).
"""
import numpy as np
import torch

FIELDS = ("steps", "clipped", "nonfinite", "last_norm", "last_coef", "max_norm_seen")
CHUNK, THREADS = 1024, 256         # AAC_CLIP_CHUNK, AAC_CLIP_THREADS


class ClippedAdam(torch.optim.Adam):
    """Adam behind ``clip_grad_norm_(params, max_norm)``; ``norms`` keeps every step's total norm.
    ``max_norm=None``: plain Adam (the norm is still recorded)."""

    def __init__(self, params, max_norm, **kw):
        super().__init__(params, **kw)
        self.max_norm, self.norms = max_norm, []

    def step(self, closure=None):
        ps = [p for g in self.param_groups for p in g["params"] if p.grad is not None]
        bound = float("inf") if self.max_norm is None else self.max_norm
        self.norms.append(float(torch.nn.utils.clip_grad_norm_(ps, bound)))
        return super().step(closure)


def sum_copies(copies, order):
    """copies [ns][n] (float32 or float64 numpy) summed in their own type: order 0 the copies in
    sequence, order 1 the four groups s % 4 each in sequence from zero, then (g0 + g1) + (g2 + g3)."""
    copies = np.asarray(copies)
    if order == 0:
        out = copies[0].copy()
        for s in range(1, copies.shape[0]):
            out = out + copies[s]
        return out
    a = [np.zeros_like(copies[0]) for _ in range(4)]
    for s in range(copies.shape[0]):
        a[s % 4] = a[s % 4] + copies[s]
    return (a[0] + a[1]) + (a[2] + a[3])


def coef_of(norm, max_norm):
    """clip_grad_norm_'s coefficient in float64: min(1, max_norm / (norm + 1e-6)), a NaN kept."""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return np.float64(1.0) if c >= 1.0 else c


def new_record():
    return dict(steps=0, clipped=0, nonfinite=0, last_norm=0.0, last_coef=0.0, max_norm_seen=0.0)


def clip_adam(copies, order, gscale, max_norm, p, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, record=None):
    """One unit's clipped Adam step ``t``.  The copies are summed and scaled in their own element type
    (what the kernels do), everything after that is float64: the norm, coef (rounded once to the element
    type, as the kernel applies it) and Adam on (gscale * g) * coef.  Returns (grad_out, norm, coef, p,
    m, v) and updates ``record`` (``new_record()``) in place."""
    copies = np.asarray(copies)
    dt = copies.dtype.type
    g = sum_copies(copies, order)
    with np.errstate(invalid="ignore", over="ignore"):
        gs = (g * dt(gscale)).astype(np.float64)
        norm = np.sqrt(np.sum(gs * gs))
        coef = coef_of(norm, max_norm)
        ga = gs * np.float64(dt(coef))
        p, m, v = (np.asarray(x, dtype=np.float64) for x in (p, m, v))
        b1, b2 = np.float64(dt(b1)), np.float64(dt(b2))
        m = b1 * m + (1.0 - b1) * ga
        v = b2 * v + (1.0 - b2) * ga * ga
        step_size = np.float64(dt(lr)) / (1.0 - b1 ** t)
        p = p - step_size * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + np.float64(dt(eps)))
    if record is not None:
        record["steps"] += 1
        record["clipped"] += int(coef < 1.0)
        record["nonfinite"] += int(not np.isfinite(norm))
        record["last_norm"], record["last_coef"] = float(norm), float(coef)
        record["max_norm_seen"] = float(np.fmax(record["max_norm_seen"], norm))
    return g, float(norm), float(coef), p, m, v


# ------------------------------------------------------------------------------- learner drivers
ATT_KEYS = ("s_own", "s_radar", "s_nei", "act", "rew", "done", "n_own", "n_radar", "n_nei")


def att_problem(N, B, E, seed, iters):
    """The data of ``learner_ref.check_one_update``: four pushes of E random transitions and, per update,
    N explicit index lists of B distinct rows.  Returns (pushes, host rows, idx[update][iteration])."""
    from oracle import learner_ref
    pushes = [learner_ref.random_transitions(E, N, seed * 100 + p) for p in range(4)]
    host = {k: torch.cat([tr[k] for tr in pushes]) for k in ATT_KEYS}
    gen = np.random.default_rng(seed)
    idx = [[torch.from_numpy(gen.choice(4 * E, size=B, replace=False).astype(np.int32)) for _ in range(N)]
           for _ in range(iters)]
    return pushes, host, idx


def att_batches(host, idx):
    out = []
    for i in idx:
        b = {k: v[i.long()].clone() for k, v in host.items()}
        b["done"] = b["done"].to(torch.float32)
        out.append(b)
    return out


def att_ref_run(actor, critic, host, idx, bounds, eps=1e-8):
    """``ref_update`` over the updates of ``idx`` with one ClippedAdam per network (bounds = (critic,
    actor) or None for plain Adam).  The nets are updated in place.  Returns (stats per update, targets
    (actor_t, critic_t), {"critic": norms, "actor": norms})."""
    import copy
    from oracle import learner_ref
    actor_t, critic_t = copy.deepcopy(actor), copy.deepcopy(critic)
    bc, ba = bounds if bounds is not None else (None, None)
    opts = (ClippedAdam(actor.parameters(), ba, lr=1e-3, eps=eps), ClippedAdam(critic.parameters(), bc, lr=1e-3, eps=eps))
    stats = []
    for it in idx:
        s, opts = learner_ref.ref_update(actor, critic, actor_t, critic_t, att_batches(host, it), opts=opts)
        stats.append(s)
    return stats, (actor_t, critic_t), {"critic": list(opts[1].norms), "actor": list(opts[0].norms)}


def split_bounds(norms):
    """A (critic, actor) pair of bounds from the norms of an UNCLIPPED reference run (never from the code
    under test): per network the geometric mean of the smallest and the largest norm, so that the largest
    step is clipped and -- as long as clipping does not lift every later norm above it -- the smallest is
    not.  The tests assert that both outcomes really occur."""
    return tuple(float(np.sqrt(min(norms[k]) * max(norms[k]))) for k in ("critic", "actor"))
