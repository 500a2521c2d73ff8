"""Neighbour counts for the attention kernels and agent counts for the ATT learner: which K = N - 1
hits which template instance, and the inputs to run them with.

This module restates the host dispatch of csrc/aac_learn.hip and csrc/aac_fused.hip in Python
(``instance``, ``kernel``, ``enc_instance``), lists the instances each family compiles, and names the
cases the GPU tests parametrize over; tests/test_attn_cases_cpu.py keeps the lists honest.

Attention families (K neighbour slots held in registers, one template instance per slot count):
  attn_fwd, attn_bwd            aac_attn_fwd / _bwd (ops.masked_attention, the autograd learner)   per-row <4|8|16|32>
  attn_train_fwd, _bwd          aac_attn_train_fwd / _bwd[_wn] (the fused learner's attention)      per-row <4|8|16|32>, MFMA <4|8>
  attn_block                    aac_attn_block (inference)                                          per-row <4|8|16|32>, MFMA <4>
K <= 4 -> <4>, K <= 8 -> <8>, K <= 16 -> <16>, else <32>; the MFMA variant takes over at K <= 8 (the
block: K <= 4) when pointers and strides are 16-byte aligned.  Every entry point refuses K < 1 and
K > 32.

aac_attn_enc_fwd (attn_enc_kernel<KM, KSO>): K <= 8, d_own <= 40, c_din <= 40; KM = 8 when K > 4 else
4; KSO = 10 when the widest staged row (d_own of an attention set, c_din of a riding job) is wider
than 24 floats, else 6.  With the model contract D0 = 6 + 4 (N - 1), Din = D0 + 2 the fused learner
and the fused act path therefore run N = 2..9: <4, 6> at N = 2..5, <8, 10> at N = 6..9, and N = 9
is the edge of all three limits (K = 8, d_own = 38, c_din = 40).  The autograd learner (fused=False)
goes through ops.masked_attention and reaches N = 33.

Seeds of the whole-update cases (``UPDATE_SEED``).  The device learner is compared with the fp32
torch-CPU restatement (oracle/learner_ref.py) at 1e-5; a seed is usable only if that restatement is
itself determined to 1e-5, i.e. if an fp64 run of the same restatement on the same weights and
batches agrees with the fp32 run within the tolerance (``restatement_gap``: Q, targets and losses in
the allclose form of check_one_update; parameters as a maximum absolute difference, which may take
no more than TOL / SEED_MARGIN, a quarter of the bound: the kernels sum in another order than torch
on the CPU and need the rest).  The rule
(``choose_seed``): the first seed of 0, 1, ..., 7 that passes with Adam eps = 1e-8; if none does, the
first that passes with eps = 1e-3 on both sides (the form test_update_b1024_matches_cpu_restatement
documents: where a gradient is rounding noise, Adam's step at eps = 1e-8 is +-lr whatever its size).
The criterion never looks at a kernel; the CPU test re-evaluates it for the recorded seeds.
"""
import functools

import numpy as np
import torch

# ------------------------------------------------------------------ accepted ranges (restated)
K_MIN, K_MAX = 1, 32                  # every attention entry point
ENC_K_MAX, ENC_DMAX = 8, 40           # aac_attn_enc_fwd: K, d_own and c_din
KSO_WIDE = 24                         # widest staged row above which KSO = 10
FUSED_N = (2, 9)                      # fused learner / act path
ATT_N = (2, 33)                       # any learner (K <= 32)


def d0_of(N):
    return 6 + 4 * (N - 1)


# ------------------------------------------------------------------ dispatch (restated)
FAMILIES = ("attn_fwd", "attn_bwd", "attn_train_fwd", "attn_train_bwd", "attn_block")
MFMA_K = {"attn_fwd": 0, "attn_bwd": 0, "attn_train_fwd": 8, "attn_train_bwd": 8, "attn_block": 4}
COMPILED = {f: {("row", km) for km in (4, 8, 16, 32)} | {("mfma", km) for km in (4, 8) if km <= MFMA_K[f]}
            for f in FAMILIES}
ROW_EDGES = (4, 8, 16)                # K <= edge takes the instance of that size


def instance(K):
    """The template instance the per-row dispatch picks."""
    assert K_MIN <= K <= K_MAX
    return 4 if K <= 4 else 8 if K <= 8 else 16 if K <= 16 else 32


def mfma_eligible(family, K, aligned=True):
    return aligned and K <= MFMA_K[family]


def kernel(family, K, aligned=True):
    """(variant, KM) of the kernel that runs: ("mfma", 4 | 8) or ("row", 4 | 8 | 16 | 32)."""
    return ("mfma", instance(K)) if mfma_eligible(family, K, aligned) else ("row", instance(K))


ENC_COMPILED = {(4, 6), (4, 10), (8, 6), (8, 10)}


def enc_accepts(K, d_own, c_din=1):
    return 1 <= K <= ENC_K_MAX and 1 <= d_own <= ENC_DMAX and 1 <= c_din <= ENC_DMAX


def enc_instance(K, dmax):
    """attn_enc_kernel<KM, KSO> for the largest K and the widest staged row of a launch."""
    assert 1 <= K <= ENC_K_MAX and 1 <= dmax <= ENC_DMAX
    return (8 if K > 4 else 4, 10 if dmax > KSO_WIDE else 6)


def fused_accepts(N):
    """Whether the fused learner's launches accept N agents (the model contract's K, D0 and Din)."""
    return N >= 2 and enc_accepts(N - 1, d0_of(N), d0_of(N) + 2)


# ------------------------------------------------------------------ named cases
# parity against fp64 torch: the K each test ran before, and the instance edges added to all three
K_EDGES = (5, 8, 9, 16, 17, 32)
K_ATTENTION = (1, 2, 4, 7, 15) + K_EDGES            # test_attention_fwd_bwd (ops.masked_attention)
K_TRAIN = (1, 4, 7, 12) + K_EDGES                   # test_attn_train_fwd_bwd_matches_autograd
K_BLOCK = (1, 4, 7, 15) + K_EDGES                   # test_attn_block_matches_reference_attention
R_PARITY = 131                                      # no multiple of 16 or 64 (the edge-row builder's R)
# guard-banded: the arena tests that were there (every 16-B condition broken in turn at K <= 8) and
# the new ones at the last slots of <8>, <16>, the first and the last of <32>
ARENA_OLD_K, ARENA_OLD_R = (1, 4, 7, 12), (1, 15, 17, 65)
ARENA_K, ARENA_R = (8, 16, 17, 32), (1, 19)
LAYOUTS = ("natural", "misaligned")                 # 16-B aligned (MFMA eligible) | bases off by one float
REFUSED_K = (0, 33)

# aac_attn_enc_fwd: (K, d_own, riding c_n, c_din, folded output layer)
ENC_OLD = [(K, 6 + 4 * K, 5, 24, False) for K in (1, 4, 7)]
ENC_CASES = [(8, 38, 9, 40, True),        # N = 9 as the plan builds it: o_d0 + 2 == c_din == 40
             (5, 26, 6, 28, False),       # N = 6, the first case on <8, 10>
             (4, 22, 6, 28, False),       # <4, 10>
             (8, 22, 3, 24, False)]       # <8, 6> at its last slot
ENC_R, ENC_ROWS = 67, 35
ENC_REFUSED = ("K", "d_own", "c_din")     # K = 9, d_own = 41, c_din = 41

# whole update against the restatement: (N, B, E, iters)
UPDATE_FUSED = [(2, 64, 64, 2), (6, 64, 64, 2), (9, 64, 64, 2)]
UPDATE_AUTOGRAD = [(10, 16, 16, 2), (33, 16, 16, 1)]
IDENTITY_N = (2, 9)                       # graph = eager, merged = serial: B = 64, three updates
FORMS_N9 = ("daob_off", "wn_off")         # launch forms at N = 9, same case and seed as (9, 64, 64, 2)
ACT_N, ACT_E = (2, 6, 9), 77
SPLIT_N, SPLIT_ROWS = (17, 33), 35        # grouped-GEMM list cut at 16 products
CONSTRUCT_REFUSED = (1, 10, 34)           # fused=True; 1 and 34 also with fused=False
CONSTRUCT_OK = [(2, True), (9, True), (10, False), (33, False)]

# (N, B, E, iters) -> (seed, Adam eps), chosen by ``choose_seed`` (see the module docstring)
UPDATE_SEED = {
    (2, 64, 64, 2): (1, 1e-8),
    (6, 64, 64, 2): (0, 1e-8),
    (9, 64, 64, 2): (1, 1e-3),        # eps = 1e-8: no seed of 0..7 within TOL / SEED_MARGIN
    (10, 16, 16, 2): (2, 1e-8),
    (33, 16, 16, 1): (1, 1e-3),       # likewise; one iteration: the restatement alone takes 1.5 s per iteration
}
TOL = 1e-5
SEED_MARGIN = 4.0        # the restatement's own fp32 error may take a quarter of the parameter bound


def covered():
    """{family: {(variant, KM): [case, ...]}} and the enc instances, over all named cases."""
    out = {f: {} for f in FAMILIES}

    def add(fams, tag, K, aligned):
        for f in fams:
            out[f].setdefault(kernel(f, K, aligned), []).append((tag, K, aligned))
    for K in K_ATTENTION:
        add(("attn_fwd", "attn_bwd"), "parity", K, True)
    for K in K_TRAIN:
        add(("attn_train_fwd", "attn_train_bwd"), "parity", K, True)
    for K in K_BLOCK:
        add(("attn_block",), "parity", K, True)
    for K in ARENA_OLD_K:
        for aligned in (True, False):
            add(("attn_train_fwd", "attn_train_bwd", "attn_block"), "arena_old", K, aligned)
    for K in ARENA_K:
        for aligned in (True, False):
            add(FAMILIES, "arena", K, aligned)
    enc = {}
    for K, d_own, c_n, c_din, fold in ENC_OLD + ENC_CASES:
        enc.setdefault(enc_instance(K, max(d_own, c_din)), []).append((K, d_own, c_n, c_din))
    return out, enc


def case_ks(family):
    """Every K a named case launches ``family`` with."""
    return sorted({K for cases in covered()[0][family].values() for _, K, _ in cases})


# ------------------------------------------------------------------ inputs
EDGE_ROWS = ("all_masked", "only_last", "only_first", "all_valid")


def plant_edge_rows(nei, at=0):
    """Rows at .. at + 3 of nei (R, K, 6) become: all neighbours masked; only slot K - 1 valid; only
    slot 0 valid; every slot valid.  Valid slots get values whose six-float sum is far from zero (the
    mask is ``sum != 0``); masked slots are exact zeros.  In place; returns nei."""
    R, K = nei.shape[:2]
    assert at + 4 <= R
    g = torch.Generator().manual_seed(1000 + K)
    full = (torch.rand(4, K, 6, generator=g) * 0.9 + 0.1) * (torch.randint(0, 2, (4, K, 1), generator=g) * 2 - 1)
    full = full.to(nei.dtype).to(nei.device)
    nei[at] = 0.0
    nei[at + 1] = 0.0
    nei[at + 1, K - 1] = full[1, K - 1]
    nei[at + 2] = 0.0
    nei[at + 2, 0] = full[2, 0]
    nei[at + 3] = full[3]
    return nei


def nei_rows(R, K, seed, frac=0.3):
    """Neighbour rows (R, K, 6), fp32 on the CPU: random values with a fraction ``frac`` of the slots
    masked, the four edge rows planted at rows 0..3 when R >= 4; R < 4 (the one-row arena case): row 0
    has only slot K - 1 valid."""
    g = torch.Generator().manual_seed(seed * 131 + K)
    nei = torch.randn(R, K, 6, generator=g)
    nei[..., 0] += (nei.sum(-1).abs() < 1e-2) * 0.5      # no valid slot whose sum a summation order could zero
    nei[torch.rand(R, K, generator=g) < frac] = 0.0
    if R >= 4:
        return plant_edge_rows(nei, 0)
    keep = nei[0, K - 1].clone()
    nei[0] = 0.0
    nei[0, K - 1] = keep if float(keep.sum().abs()) > 1e-3 else 0.5
    return nei


def valid_mask(nei):
    """The mask the kernels and the references use: the slot's six floats do not sum to zero."""
    return nei.sum(-1) != 0


# ------------------------------------------------------------------ the seed criterion (CPU only)
def _restatement(N, B, E, seed, iters, eps, dtype):
    """check_one_update's reference side alone, in ``dtype``: the weights MADDPG(seed) starts from,
    the batches its generator draws, ``iters`` ref_updates.  Returns (stats per iteration, params)."""
    from multi_agent_aac_amd.maddpg import MADDPG
    from oracle import learner_ref as LR
    D0 = d0_of(N)
    m = MADDPG([D0, 18, 6], [D0, 18, 6], 2, n_agents=N, device="cpu", seed=seed, memory_length=4 * E, batch_size=B,
               fused=False)
    nets = [LR.RefActor([D0, 18, 6], 2), LR.RefCritic([D0, 18, 6], N, 2), LR.RefActor([D0, 18, 6], 2),
            LR.RefCritic([D0, 18, 6], N, 2)]
    for net, src in zip(nets, (m.actors, m.critics, m.actors, m.critics)):
        net.load_state_dict(src.reference_state_dict())
        net.to(dtype)
    host = {k: [] for k in ("s_own", "s_radar", "s_nei", "act", "rew", "done", "n_own", "n_radar", "n_nei")}
    for p in range(4):
        tr = LR.random_transitions(E, N, seed * 100 + p)
        for k in host:
            host[k].append(tr[k])
    host = {k: torch.cat(v) for k, v in host.items()}
    gen = np.random.default_rng(seed)
    opts = (torch.optim.Adam(nets[0].parameters(), lr=1e-3, eps=eps), torch.optim.Adam(nets[1].parameters(), lr=1e-3, eps=eps))
    stats = []
    for _ in range(iters):
        idx = [torch.from_numpy(gen.choice(4 * E, size=B, replace=False).astype(np.int32)) for _ in range(N)]
        batches = [{k: v[i.long()].to(dtype) for k, v in host.items()} for i in idx]
        st, opts = LR.ref_update(*nets, batches, opts=opts)
        stats += [(lq, la, q.squeeze(1), tg) for lq, la, q, tg in st]
    return stats, [p.detach() for net in nets for p in net.parameters()]


@functools.lru_cache(maxsize=None)
def restatement_gap(N, B, E, seed, iters, eps):
    """(stat_ok, param gap) of the fp32 against the fp64 restatement: ``stat_ok`` in the allclose /
    relative-loss form check_one_update applies at TOL, the largest parameter difference."""
    s32, p32 = _restatement(N, B, E, seed, iters, eps, torch.float32)
    s64, p64 = _restatement(N, B, E, seed, iters, eps, torch.float64)
    ok = True
    for (lq, la, q, tg), (rlq, rla, rq, rtg) in zip(s32, s64):
        ok &= bool(torch.allclose(q.double(), rq, atol=TOL, rtol=TOL) and torch.allclose(tg.double(), rtg, atol=TOL, rtol=TOL))
        ok &= abs(lq - rlq) <= TOL * max(1.0, abs(rlq)) and abs(la - rla) <= TOL * max(1.0, abs(rla))
    return ok, max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64))


def seed_passes(N, B, E, seed, iters, eps):
    ok, gap = restatement_gap(N, B, E, seed, iters, eps)
    return ok and gap <= TOL / SEED_MARGIN


def choose_seed(N, B, E, iters, seeds=range(8)):
    for eps in (1e-8, 1e-3):
        for seed in seeds:
            if seed_passes(N, B, E, seed, iters, eps):
                return seed, eps
    raise AssertionError(f"no usable seed for N {N} B {B} E {E} iters {iters}")
