"""The attention case table (tests/attn_cases.py): every compiled template instance of every kernel
family is hit by a named case, both sides of every ``<=`` of the dispatch are hit, the input builders
produce the edge rows for every K, the restated ranges are those of ``fused.py`` and of the
constructor, and the recorded seeds meet the CPU-only criterion they were chosen by."""
import pytest
import torch

from tests import attn_cases as C


def test_restated_dispatch():
    assert [C.instance(K) for K in (1, 4, 5, 8, 9, 16, 17, 32)] == [4, 4, 8, 8, 16, 16, 32, 32]
    assert C.kernel("attn_train_fwd", 8) == ("mfma", 8) and C.kernel("attn_train_fwd", 8, aligned=False) == ("row", 8)
    assert C.kernel("attn_train_bwd", 9) == ("row", 16)
    assert C.kernel("attn_block", 4) == ("mfma", 4) and C.kernel("attn_block", 5) == ("row", 8)
    assert C.kernel("attn_fwd", 3) == ("row", 4) and C.kernel("attn_bwd", 32) == ("row", 32)
    assert sum(len(v) for v in C.COMPILED.values()) == 4 + 4 + 6 + 6 + 5
    # the model contract through the fused launch: N = 2..5 on <4, 6>, 6..9 on <8, 10>, nothing else accepted
    accepted = [N for N in range(0, 40) if C.fused_accepts(N)]
    assert accepted == list(range(C.FUSED_N[0], C.FUSED_N[1] + 1)) == list(range(2, 10))
    inst = {N: C.enc_instance(N - 1, C.d0_of(N) + 2) for N in accepted}
    assert [inst[N] for N in accepted] == [(4, 6)] * 4 + [(8, 10)] * 4
    assert (C.FUSED_N[1] - 1, C.d0_of(9), C.d0_of(9) + 2) == (C.ENC_K_MAX, 38, C.ENC_DMAX)      # N = 9: all three limits
    assert C.ATT_N == (C.K_MIN + 1, C.K_MAX + 1)


@pytest.mark.parametrize("family", C.FAMILIES)
def test_every_compiled_instance_has_a_case(family):
    cov, _ = C.covered()
    assert set(cov[family]) == C.COMPILED[family], (family, C.COMPILED[family] - set(cov[family]))
    # and by a case this work added, wherever the instance had never run (<32> of every family)
    assert any(tag != "arena_old" for tag, K, al in cov[family][("row", 32)])


@pytest.mark.parametrize("family", C.FAMILIES)
def test_both_sides_of_every_comparison(family):
    ks = C.case_ks(family)
    for edge in C.ROW_EDGES:                                      # K <= 4 | 8 | 16 of the per-row dispatch
        assert edge in ks and edge + 1 in ks, (family, edge)
        assert C.instance(edge) != C.instance(edge + 1)
    assert C.K_MIN in ks and C.K_MAX in ks                        # the accepted ends ...
    assert C.REFUSED_K == (C.K_MIN - 1, C.K_MAX + 1)              # ... and the first refused value on each side
    cov, _ = C.covered()
    m = C.MFMA_K[family]
    if m:
        # K <= m of the MFMA branch, and its alignment condition both ways at the last eligible K
        lo = [c for c in cov[family][("mfma", m)] if c[1] == m]
        hi = [c for c in cov[family][("row", C.instance(m + 1))] if c[1] == m + 1 and c[2]]
        assert lo and hi, (family, m)
        assert any(c[1] == m and not c[2] for c in cov[family][("row", m)]), (family, m)


def test_parity_lists_extend_the_old_ones():
    assert C.K_ATTENTION[:5] == (1, 2, 4, 7, 15) and C.K_TRAIN[:4] == (1, 4, 7, 12) and C.K_BLOCK[:4] == (1, 4, 7, 15)
    for ks in (C.K_ATTENTION, C.K_TRAIN, C.K_BLOCK):
        assert set(C.K_EDGES) <= set(ks) and len(set(ks)) == len(ks)
    assert C.K_EDGES == (5, 8, 9, 16, 17, 32) and C.ARENA_K == (8, 16, 17, 32) and C.ARENA_R == (1, 19)
    assert C.R_PARITY % 16 and C.R_PARITY % 64


def test_enc_cases_cover_every_instance_and_limit():
    _, enc = C.covered()
    assert set(enc) == C.ENC_COMPILED
    new = {C.enc_instance(K, max(d, cd)) for K, d, cn, cd, fold in C.ENC_CASES}
    assert new == {(8, 10), (4, 10), (8, 6)}                      # <4, 6> is the one the old cases ran
    assert all(C.enc_instance(K, max(d, cd)) == (4, 6) or K == 7 for K, d, cn, cd, fold in C.ENC_OLD)
    assert C.ENC_CASES[0] == (C.ENC_K_MAX, C.ENC_DMAX - 2, 9, C.ENC_DMAX, True)
    # both sides of K > 4 and of dmax > 24
    assert {K for K, *_ in C.ENC_CASES} >= {4, 5, 8}
    assert {max(d, cd) for K, d, cn, cd, fold in C.ENC_OLD + C.ENC_CASES} >= {24, 28, 40}
    assert all(C.enc_accepts(K, d, cd) for K, d, cn, cd, fold in C.ENC_CASES)
    assert not C.enc_accepts(9, 38, 40) and not C.enc_accepts(8, 41, 40) and not C.enc_accepts(8, 38, 41)
    assert C.ENC_R % 16 and C.ENC_ROWS % 16


@pytest.mark.parametrize("R", [C.R_PARITY, 19])
def test_builders_make_the_edge_rows_for_every_k(R):
    for K in range(C.K_MIN, C.K_MAX + 1):
        nei = C.nei_rows(R, K, seed=3)
        assert nei.shape == (R, K, 6) and nei.dtype == torch.float32
        for m in (C.valid_mask(nei), C.valid_mask(nei.double())):
            assert not m[0].any()                                               # all masked
            assert m[1].nonzero().flatten().tolist() == [K - 1]                 # only the last slot
            assert m[2].nonzero().flatten().tolist() == [0]                     # only the first
            assert m[3].all()                                                   # fully valid
            if K >= 4:
                rest = m[4:]
                assert rest.any() and not rest.all()                            # random masking elsewhere
        # the mask is safe: a valid slot's sum is far from zero, a masked slot is exact zeros, and the
        # reference's mean-based mask agrees
        s = nei.double().sum(-1)
        assert float(s[C.valid_mask(nei)].abs().min()) > 1e-4
        assert float(nei[~C.valid_mask(nei)].abs().max()) == 0.0
        assert torch.equal(nei.double().mean(-1) != 0, C.valid_mask(nei))
        # planting into rows of another tensor (the parity tests plant at row 10 of their own inputs)
        other = C.plant_edge_rows(torch.randn(20, K, 6), at=10)
        mo = C.valid_mask(other)
        assert not mo[10].any() and mo[11].sum() == 1 and mo[11, K - 1] and mo[12].sum() == 1 and mo[12, 0] and mo[13].all()


def test_one_row_builder_keeps_the_last_slot():
    for K in range(C.K_MIN, C.K_MAX + 1):
        m = C.valid_mask(C.nei_rows(1, K, seed=3))
        assert m.shape == (1, K) and m[0].nonzero().flatten().tolist() == [K - 1]


def test_ranges_agree_with_the_package():
    from multi_agent_aac_amd import fused
    assert (fused.FUSED_N_MIN, fused.FUSED_N_MAX) == C.FUSED_N and (fused.N_MIN, fused.N_MAX) == C.ATT_N
    assert fused.ATTN_K_MAX == C.K_MAX and (fused.ENC_K_MAX, fused.ENC_DMAX) == (C.ENC_K_MAX, C.ENC_DMAX)
    for N in range(-1, 40):
        for fz in (True, False):
            ok = (C.fused_accepts(N) if fz else C.ATT_N[0] <= N <= C.ATT_N[1])
            if ok:
                fused.check_agents(N, fz)
            else:
                with pytest.raises(ValueError):
                    fused.check_agents(N, fz)
    assert fused.GEMM_MAX == 16 and all(N > fused.GEMM_MAX for N in C.SPLIT_N)


@pytest.mark.parametrize("N", C.CONSTRUCT_REFUSED)
def test_constructor_refuses_unsupported_counts(N):
    from multi_agent_aac_amd.maddpg import MADDPG
    D0 = C.d0_of(max(N, 1))
    with pytest.raises(ValueError, match="fused=False" if N == 10 else "supports 2..33"):
        MADDPG([D0, 18, 6], [D0, 18, 6], 2, n_agents=N, device="cpu", seed=0)
    if N != 10:
        with pytest.raises(ValueError, match="supports 2..33"):
            MADDPG([D0, 18, 6], [D0, 18, 6], 2, n_agents=N, device="cpu", seed=0, fused=False)


@pytest.mark.parametrize("N,fz", C.CONSTRUCT_OK)
def test_constructor_accepts_the_supported_ends(N, fz):
    from multi_agent_aac_amd.maddpg import MADDPG
    m = MADDPG([C.d0_of(N), 18, 6], [C.d0_of(N), 18, 6], 2, n_agents=N, device="cpu", seed=0, fused=fz)
    assert m.n_agents == N and m.fused == fz


def test_update_cases_have_seeds():
    cases = C.UPDATE_FUSED + C.UPDATE_AUTOGRAD
    assert [c[:2] for c in C.UPDATE_FUSED] == [(2, 64), (6, 64), (9, 64)] and all(c[2:] == (64, 2) for c in C.UPDATE_FUSED)
    assert [c[:3] for c in C.UPDATE_AUTOGRAD] == [(10, 16, 16), (33, 16, 16)]
    assert set(C.UPDATE_SEED) == set(cases)
    assert all(eps in (1e-8, 1e-3) for _, eps in C.UPDATE_SEED.values())
    assert C.IDENTITY_N == (2, 9) and C.ACT_N == (2, 6, 9) and C.ACT_E == 77 and C.SPLIT_N == (17, 33)


@pytest.mark.parametrize("case", C.UPDATE_FUSED + C.UPDATE_AUTOGRAD, ids=lambda c: "N%d-B%d" % c[:2])
def test_recorded_seeds_meet_the_criterion(case):
    """The fp32 and the fp64 restatement agree for the recorded (seed, eps): statistics within TOL,
    parameters within TOL / SEED_MARGIN.  (Which seed is the *first* to pass is the rule the seeds
    were chosen by, ``choose_seed``; re-running that search is left to whoever changes a case.)"""
    N, B, E, iters = case
    seed, eps = C.UPDATE_SEED[case]
    ok, gap = C.restatement_gap(N, B, E, seed, iters, eps)
    assert ok and gap <= C.TOL / C.SEED_MARGIN, (case, seed, eps, ok, gap)
