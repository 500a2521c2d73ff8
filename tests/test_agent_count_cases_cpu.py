"""The agent-count case table (tests/agent_count_cases.py) covers both sides of every N-dependent
branch of the env kernels, its Python restatements give the values the kernel comments state, the LDS
bounds the kernels derive by hand hold for every accepted N, and every crowded N > 64 input really
depends on the agents past the first 64."""
import numpy as np
import pytest

from tests import agent_count_cases as C


def test_restatements_match_the_stated_values():
    assert [C.epb_of(3, N) for N in (2, 9, 12, 13, 24, 25, 256)] == [12, 2, 2, 1, 1, 1, 1]
    assert C.epb_of(4096, 8) == 4 and C.epb_of(4096, 5) == 4          # raised until 1024 workgroups hold E
    assert C.epb_of(262144, 5) == 10                                  # epb_for(50) once E / epb >= 1024
    assert C.epb_of(*C.EPB_GROWTH) == 13 and C.branches("att", *C.EPB_GROWTH)["epb_grown"]
    assert [C.staged("att", 3, N) for N in (12, 16, 17)] == [False, True, False]
    assert 16 * C.row_floats("att", 16) == 2496 and 24 * C.row_floats("att", 12) == 2784
    assert [C.staged("wgru", 3, N) for N in (20, 21)] == [True, False]
    assert 20 * C.row_floats("wgru", 20) == 2400


@pytest.mark.parametrize("branch,values", [
    ("radar_chunks", (1, 2, 3, 4)), ("agent_waves", (1, 2, 3, 4)), ("spec", (True, False)),
    ("late_copy", (True, False)), ("prefetch_all", (True, False)), ("staged", (True, False)),
    ("epb", (12, 2, 1)), ("epb_grown", (True, False)), ("ragged", (True,))])
def test_every_branch_has_a_case_on_each_side(branch, values):
    for v in values:
        assert C.SIDES[branch].get(v), (branch, v)


def test_straddles():
    """The pairs a reader expects, each next to its threshold."""
    b = lambda v, N: C.branches(v, C.small_E(N), N)
    parity = {(v, N) for v, N, *_ in C.PARITY}
    for v, lo, hi, key in (("att", 16, 17, "staged"), ("wgru", 20, 21, "staged"), ("att", 84, 85, "spec"),
                           ("att", 64, 65, "radar_chunks"), ("att", 64, 65, "agent_waves"),
                           ("wgru", 64, 65, "prefetch_all"), ("att", 192, 193, "late_copy")):
        assert b(v, lo)[key] != b(v, hi)[key], (v, lo, hi, key)
        assert (v, hi) in parity and ((v, lo) in parity or lo == 192), (v, lo, hi)
    assert ("att", C.N_MAX) in parity and ("wgru", C.N_MAX) in parity
    assert b("att", 12)["staged"] is False and b("att", 12)["epb"] == 2     # unstaged below the staged 16
    # the fused tail: ring pushes need staged rows; the no-ring cases cross spec and the agent-free wave
    assert all(C.staged(v, 40, N) for v, N in C.TAIL_RING)
    assert not any(C.staged(v, 40, N) for v, N in C.TOO_WIDE)
    spec = {C.branches(v, 40, N)["spec"] for v, N in C.TAIL_NO_RING}
    free = {C.branches(v, 40, N)["late_copy"] for v, N in C.TAIL_NO_RING}
    assert spec == {True, False} and free == {True, False}
    # the parity cases were not thinned out
    assert {N for v, N, *_ in C.PARITY if v == "att"} == set(C.ATT_N) and len(C.ATT_N) == 14
    assert {N for v, N, *_ in C.PARITY if v == "wgru"} == set(C.WGRU_N) and len(C.WGRU_N) == 10
    assert {(N, m) for v, N, m, *_ in C.PARITY if v == "att" and N in (2, 65, 256)} >= \
        {(N, m) for N in (2, 65, 256) for m in (0, 1)}
    assert {N for v, N, m, td, tr in C.PARITY if td} == {2, 9, 65}
    assert {N for v, N, m, td, tr in C.PARITY if v == "att" and tr} >= {2, 65, 256}
    assert {N for N, _ in C.CROWDED} == {9, 64, 65, 130, 256} and {m for _, m in C.CROWDED} == {0, 2}
    assert C.BANK_DRAW_N == (2, 64, 85, 256)


def test_hand_derived_lds_bounds_hold_for_every_count():
    """spec_draw keeps episode / map words at S.idx[nag + epb + lq] and the drawn starts as double2
    in S.rmin from (nag + 1) & ~1 on, both arrays of BLOCK entries; a thread's flagged-ray mask has
    one bit per 256 work items.  Checked for every N and every epb the create rule can choose."""
    for N in range(2, C.N_MAX + 1):
        for epb in range(C.epb_for(24, N), C.epb_for(50, N) + 1):
            nag = epb * N
            assert nag <= C.BLOCK
            assert (nag * 18 + C.BLOCK - 1) // C.BLOCK <= 32
            if nag <= C.SPEC_MAX_AG:
                assert nag + 2 * epb <= C.BLOCK
                assert ((nag + 1) & ~1) + 2 * nag <= C.BLOCK
    assert ((C.SPEC_MAX_AG + 1) & ~1) + 2 * C.SPEC_MAX_AG == 252      # why 84: 85 would end at 256, 86 past it


def test_uam_counts_cover_idle_lanes_and_the_full_wave():
    idle = {N: 64 - (64 // N) * N for N in C.UAM_N}
    assert idle == {7: 1, 33: 31, 63: 1, 64: 0} and 64 // 7 == 9 and C.UAM_N_MAX in C.UAM_N


def test_placed_od_is_a_legal_od(occ):
    st, wps, cnt = C.placed_od(occ, 3, 256, seed=1)
    d = np.linalg.norm(st[:, :, None] - st[:, None], axis=-1) + np.eye(256) * 99
    assert d.min() > 5.0                                              # starts more than 2 pB apart
    assert cnt.min() >= 1 and cnt.max() <= 3
    e, i = np.indices(cnt.shape)
    assert np.array_equal(wps[e, i, cnt - 1], wps[:, :, -1])          # padded with the goal
    assert (d < 10).sum() > 256                                       # close enough for penalties and radar hits


@pytest.mark.parametrize("N", sorted({N for N, _ in C.CROWDED if N > 64}))
def test_crowded_inputs_depend_on_agents_past_64(occ, N):
    pos = C.crowded_state(8 if N < 256 else 4, N, C.CROWDED_SEED[N])
    got = C.second_chunk_matters(occ, pos)
    assert sorted(got) == list(range(64, N, 64)) and all(got.values()), got
