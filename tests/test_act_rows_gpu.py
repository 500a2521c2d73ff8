"""The act-path kernels past their up-front noise window, and every row's noise against noise_ref.

actor_head_ws_kernel (csrc/aac_learn.hip), gru_actor_fwd_kernel<2, false> (csrc/aac_gru.hip) and
uam_actor_ws_kernel<NT> (csrc/aac_uam_actor.hip) launch at most one workgroup per CU, walk their row
blocks with stride gridDim (prefetching the next block) and draw the noise of the workgroup's first
8 blocks up front into LDS; block index >= 8 of a workgroup takes an inline row_noise call instead.
The up-front window is therefore 8 x grid x rows-per-block rows (``window`` below restates each
launcher's grid formula).  The shapes here are the smallest that put every boolean of that
structure in both directions: up-front / inline noise, a prefetched next block / the last block,
a full / a partial block.

Noise checks are on every row: the fp32 kernels' noise_out within 1 ulp of noise_ref.noise32 with
the launch's epoch and the noisy action bit-equal to clamp(plain + noise_out) in float32, plain
being the same kernel's noisy=False output; the float64 UAM output within 1e-12 of
clip(plain + noise_ref.noise64).  Counters start at 41, so an epoch of 0 would not pass; a
counter compared as a whole 64-bit word has its arrival half back at 0.

The value references and tolerances are those of the neighbouring tests: ATT head / output layer
against the float64 restatement at 1e-5 (test_learner_gpu.test_actor_pth_roundtrip), the GRU act
against gru_ref.ref_gru_act at 2e-5 (test_gru_gpu), the UAM actor against the float64 module at
1e-13 (test_uam_learner_gpu)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import gru_ref
from tests import noise_ref
from tests.arena import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB = 8                  # AH_NB, GNB = 256 / GROWS at GNT = 2, NBN: blocks of a workgroup with up-front noise
CUS = 256               # the launchers' cap: one workgroup per CU
C0 = 41                 # the noise counter before the first noisy launch of a case


def window(rows, rpb, grid):
    """(grid, up-front window in rows, block index within its workgroup of every row) of a
    weights-stationary launch over ``rows`` rows in blocks of ``rpb`` on ``grid`` workgroups."""
    nblk = (rows + rpb - 1) // rpb
    assert grid == min(nblk, grid)
    kb = (np.arange(rows) // rpb) // grid
    return NB * grid * rpb, kb


def paths(rows, rpb, grid):
    """The structure's booleans over the launch: rows with inline noise, the largest block index of
    a workgroup, the number of workgroups that reach it, whether the last block is partial."""
    win, kb = window(rows, rpb, grid)
    nblk = (rows + rpb - 1) // rpb
    return dict(window=win, fallback_rows=int((kb >= NB).sum()), max_kb=int(kb.max()),
                wgs_at_max=int(nblk - kb.max() * grid), partial=rows % rpb != 0, nblk=nblk)


def _counter(v=C0):
    return torch.full((1,), v, dtype=torch.int64, device=DEV)


def _episodes(E, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, hi, (E,), dtype=torch.int32, generator=g)


def _check_noisy32(plain, act, noise, want):
    """fp32 kernels: noise within 1 ulp of the restatement, action = clamp(plain + noise) to the bit."""
    np.testing.assert_array_max_ulp(noise, want, maxulp=1)
    np.testing.assert_array_equal(act.view(np.int32), np.clip(plain + noise, np.float32(-1), np.float32(1)).view(np.int32))


# ============================================================================ ATT head (aac_actor_head_ws)
AH_RPB = 16
# (R, N): fallback rows, largest block index of a workgroup, workgroups reaching it, partial last block
HEAD_CASES = {
    (1, 1): (0, 0, 1, True),              # one workgroup, one row
    (15, 1): (0, 0, 1, True),
    (16, 1): (0, 0, 1, False),
    (17, 1): (0, 0, 2, True),             # two workgroups, the second with one row
    (4095, 1): (0, 0, 256, True),         # 256 blocks: every CU one block, no prefetch
    (4097, 1): (0, 1, 1, True),           # 257 blocks: workgroup 0 prefetches a one-row second block
    (32768, 1): (0, 7, 256, False),       # exactly the window: block index 7 everywhere, the last up-front slot
    (32769, 1): (1, 8, 1, True),          # one row past it: row 32768 = block index 8 of workgroup 0, inline noise
    (36905, 5): (4137, 9, 3, True),       # 2307 blocks: index 8 everywhere, index 9 on workgroups 0-2, 9 rows in the last
}


def _head_weights(seed):
    g = torch.Generator().manual_seed(seed)
    wm = torch.randn(256, 192, generator=g) / 192 ** 0.5
    bm = torch.randn(256, generator=g) * 0.1
    wa = torch.randn(2, 256, generator=g) / 16
    ba = torch.randn(2, generator=g) * 0.1
    return wm, bm, wa, ba


@pytest.mark.parametrize("ldc", [192, 196])
@pytest.mark.parametrize("R,N", list(HEAD_CASES))
def test_actor_head_ws_rows_and_noise(native_lib, R, N, ldc):
    """aac_actor_head_ws called directly, every operand the launch reads by row or writes carved from
    the arena (cat rows ldc apart: the row gaps and guards hold the canary; act and noise_out: every
    row < R written, nothing else).  Grid = min(ceil(R / 16), 256), window = 8 x grid x 16 = 32 768
    rows at 256 workgroups.  R = 32 768 ends on block index 7 of every workgroup (the last up-front
    slot); R = 32 769 puts row 32 768 alone into block 2048 = index 8 of workgroup 0 (inline noise, no
    prefetch after it); R = 36 905 = 5 x 7381 has 2307 blocks = 9 x 256 + 3, so every workgroup runs
    index 8 inline, workgroups 0-2 index 9, and block 2306 holds 9 rows: 4137 rows take inline noise."""
    from multi_agent_aac_amd import ops
    want_fb, want_kb, want_wgs, want_partial = HEAD_CASES[(R, N)]
    grid = min((R + AH_RPB - 1) // AH_RPB, CUS)                    # aac_actor_head_ws: wg = min(nblk, 256)
    p = paths(R, AH_RPB, grid)
    assert (p["fallback_rows"], p["max_kb"], p["wgs_at_max"], p["partial"]) == (want_fb, want_kb, want_wgs, want_partial)
    assert p["window"] == NB * grid * AH_RPB and (R > p["window"]) == (want_fb > 0)
    if R == 32768:
        assert R == p["window"]
    wm, bm, wa, ba = _head_weights(R)
    g = torch.Generator().manual_seed(R + ldc)
    x = torch.randn(R, 192, generator=g)
    h = torch.relu(x.double() @ wm.double().t() + bm.double())
    ref = torch.tanh(h @ wa.double().t() + ba.double())
    dw = [t.to(DEV).contiguous() for t in (wm, bm, wa, ba)]
    E = R // N
    ep = _episodes(E, 9000, R)
    ep_d = ep.to(DEV)
    ar = Arena(R * ldc + 6 * (2 * R + 64) + 64, torch.float32, DEV, max_ld=ldc)
    cat = ar.take(R, 192, ld=ldc, data=x, name="cat")
    a_plain, a1, n1, a2, n2 = (ar.take(R, 2, name=k) for k in ("act plain", "act 1", "noise 1", "act 2", "noise 2"))
    ctr = _counter()
    catv = cat.view
    assert catv.stride(0) == ldc and catv.data_ptr() == cat.ptr

    def launch(act, nz, noisy):
        ar.inside_mat(cat.ptr, R, 192, ldc, "cat")
        ar.inside(act.ptr, 2 * R, "act")
        ar.inside(nz.ptr if nz else 0, 2 * R, "noise_out")
        ops.actor_head_ws(catv, *[t.data_ptr() for t in dw], act.view, N, ep_d, 8000, 1.0, 0.05, 99, ctr,
                          nz.view if nz else None, noisy=noisy)

    launch(a_plain, None, False)
    ar.check(writable=[a_plain])                       # the noise-free launch: one output, no counter
    assert int(ctr.item()) == C0
    plain = a_plain.get().numpy()
    np.testing.assert_allclose(plain.astype(np.float64), ref.numpy(), atol=1e-5, rtol=1e-5)
    ar.freeze([a_plain])
    rows = np.arange(R)
    for k, (act, nz) in enumerate(((a1, n1), (a2, n2))):
        launch(act, nz, True)
        ar.check(writable=[act, nz])
        ar.freeze([act, nz])
        assert int(ctr.item()) == C0 + k + 1           # the whole word: arrivals back at 0
        want = noise_ref.noise32(99, C0 + k, rows, N, ep.numpy(), 8000, 1.0, 0.05)
        _check_noisy32(plain, act.get().numpy(), nz.get().numpy(), want)


@pytest.mark.parametrize("R,N", [(1, 1), (15, 1), (16, 1), (17, 1), (63, 1), (64, 1), (65, 1), (5 * 1001, 5)])
def test_actor_out_noise_rows(native_lib, R, N):
    """aac_actor_out_noise: a wave owns 16 rows and a workgroup 64, rows past R load row 0 (the
    arena's canary rows behind ha would make a NaN of any row that read them).  Outputs in the arena;
    every row's noise against the restatement over two launches."""
    from multi_agent_aac_amd import ops
    _, _, wa, ba = _head_weights(7)
    g = torch.Generator().manual_seed(R)
    ha = torch.relu(torch.randn(R, 256, generator=g))
    ref = torch.tanh(ha.double() @ wa.double().t() + ba.double())
    wa_d, ba_d = wa.to(DEV).contiguous(), ba.to(DEV)
    ep = _episodes(R // N, 9000, R + 1)
    ep_d = ep.to(DEV)
    ar = Arena(R * 256 + 6 * (2 * R + 64) + 64, torch.float32, DEV, max_ld=256)
    H = ar.take(R, 256, data=ha, name="ha")
    a_plain, a1, n1, a2, n2 = (ar.take(R, 2, name=k) for k in ("act plain", "act 1", "noise 1", "act 2", "noise 2"))
    ctr = _counter()

    def launch(act, nz, noisy):
        ar.inside(H.ptr, R * 256, "ha")
        ar.inside(act.ptr, 2 * R, "act")
        ar.inside(nz.ptr if nz else 0, 2 * R, "noise_out")
        ops.actor_out_noise(H.view, wa_d.data_ptr(), ba_d.data_ptr(), act.view, N, ep_d, 8000, 1.0, 0.05, 99, ctr,
                            nz.view if nz else None, noisy=noisy)

    launch(a_plain, None, False)
    ar.check(writable=[a_plain])
    assert int(ctr.item()) == C0
    plain = a_plain.get().numpy()
    np.testing.assert_allclose(plain.astype(np.float64), ref.numpy(), atol=1e-5, rtol=1e-5)
    ar.freeze([a_plain])
    rows = np.arange(R)
    for k, (act, nz) in enumerate(((a1, n1), (a2, n2))):
        launch(act, nz, True)
        ar.check(writable=[act, nz])
        ar.freeze([act, nz])
        assert int(ctr.item()) == C0 + k + 1
        want = noise_ref.noise32(99, C0 + k, rows, N, ep.numpy(), 8000, 1.0, 0.05)
        _check_noisy32(plain, act.get().numpy(), nz.get().numpy(), want)


# ============================================================================ GRU act (aac_gru_actor_fwd)
GRU_RPB = 32            # GROWS = 16 GNT, GNT = 2 on the act path
# (E, N): envs with inline noise, largest block index, workgroups of one agent reaching it, partial last block
GRU_CASES = {
    (17, 8): (0, 0, 1, True),
    (1023, 8): (0, 0, 32, True),          # 32 blocks on G = 32 workgroups per agent: no second block
    (1025, 8): (0, 1, 1, True),           # 33 blocks: workgroup 0 of each agent runs a one-env second block
    (8192, 8): (0, 7, 32, False),         # exactly the window: the last up-front slot everywhere
    (8193, 8): (1, 8, 1, True),           # env 8192 alone in block 256 = index 8 of workgroup 0: inline noise
    (9307, 8): (1115, 9, 3, True),        # 291 blocks = 9 x 32 + 3: index 8 everywhere, index 9 on three, 27 envs last
    (2721, 3): (0, 1, 1, True),           # G = 85 (not a power of two): 86 blocks, one env in the last
}
_gru_models = {}


def _gru_model(N):
    from multi_agent_aac_amd.gru import MADDPG
    if N not in _gru_models:
        m = MADDPG([6, 18, 6], [6, 18, 6], 2, 64, 10, n_agents=N, device=DEV, seed=20 + N, batch_size=64)
        actors = [gru_ref.RefGRUActor([6, 18, 6], 2) for _ in range(N)]
        for i in range(N):
            actors[i].load_state_dict({k: v.cpu() for k, v in m.actors[i].state_dict().items()})
        _gru_models[N] = (m, actors)
    return _gru_models[N]


@pytest.fixture(scope="module", autouse=True)
def _drop_models():
    yield
    _gru_models.clear()


@pytest.mark.parametrize("own_width", [6, 34])
@pytest.mark.parametrize("E,N", list(GRU_CASES))
def test_gru_act_ws_rows_and_noise(native_lib, monkeypatch, E, N, own_width):
    """gru.MADDPG.act with the weights-stationary launch on (gru_actor_fwd_kernel<2, false>: 32 envs
    per block, G = min(ceil(E / 32), 256 // N) workgroups per agent, window = 8 x G x 32 envs: 8192 at
    N = 8).  E = 8192 ends on block index 7; E = 8193 puts env 8192 into block 256 = index 8 of
    workgroup 0; E = 9307 has 291 blocks = 9 x 32 + 3: index 8 inline on every workgroup, index 9 on
    three, 27 envs in block 290: 1115 envs (x 8 agents) take inline noise.  N = 3 gives G = 85.
    hout and noise_out are arena regions; actions and hout against gru_ref.ref_gru_act at 2e-5."""
    from multi_agent_aac_amd import gru
    monkeypatch.setattr(gru, "ACT_WS", True)
    want_fb, want_kb, want_wgs, want_partial = GRU_CASES[(E, N)]
    blocks = (E + GRU_RPB - 1) // GRU_RPB
    G = max(1, min(blocks, CUS // N))                               # aac_gru_actor_fwd: workgroups per agent
    p = paths(E, GRU_RPB, G)
    assert (p["fallback_rows"], p["max_kb"], p["wgs_at_max"], p["partial"]) == (want_fb, want_kb, want_wgs, want_partial)
    assert p["window"] == NB * G * GRU_RPB and (E > p["window"]) == (want_fb > 0)
    if E == 8192:
        assert E == p["window"]
    m, actors = _gru_model(N)
    m._acts.clear()
    tr = gru_ref.random_gru_transitions(E, N, E + own_width, D0=6)
    own = torch.zeros(E, N, own_width)
    own[:, :, :6] = tr["s_own"]
    if own_width > 6:
        own[:, :, 6:] = 1e30                         # columns the networks do not read
    own_d, radar_d, h_d = own.to(DEV), tr["s_radar"].to(DEV), tr["h_cur"].to(DEV)
    ep = _episodes(E, 9000, E)
    ep_d = ep.to(DEV)
    ar = Arena(E * N * 64 + 2 * (2 * E * N + 64) + 64, torch.float32, DEV, max_ld=64)
    hout = ar.take(E * N, 64, name="hout")
    nzs = [ar.take(E * N, 2, name=f"noise {k}") for k in range(2)]
    hv = hout.view.view(E, N, 64)
    assert hv.is_contiguous() and hv.data_ptr() == hout.ptr
    a, hn = m.act(own_d, radar_d, h_d, noisy=False, h_out=hv)
    assert next(iter(m._acts.values())).ws
    plain = a.cpu().numpy().reshape(-1, 2).copy()
    ar.check(writable=[hout])
    ra, rh = gru_ref.ref_gru_act(actors, tr["s_own"], tr["s_radar"], tr["h_cur"], 6)
    np.testing.assert_allclose(plain.reshape(E, N, 2), ra, atol=2e-5)
    np.testing.assert_allclose(hout.get().view(E, N, 64), rh, atol=2e-5)
    hout_plain = hout.get()
    m.noise_counter.fill_(C0)
    rows = np.arange(E * N)
    for k, nz in enumerate(nzs):
        nv = nz.view.view(E, N, 2)
        assert nv.data_ptr() == nz.ptr
        a, _ = m.act(own_d, radar_d, h_d, episode=ep_d, noisy=True, noise_out=nv, h_out=hv)
        act = a.cpu().numpy().reshape(-1, 2).copy()
        ar.check(writable=[hout, nz])
        ar.freeze([nz])
        assert int(m.noise_counter.item()) == C0 + k + 1
        assert torch.equal(hout.get(), hout_plain)   # the hidden state does not see the noise
        want = noise_ref.noise32(m.noise_seed, C0 + k, rows, N, ep.numpy(), 8000, 1.0, 0.03)
        _check_noisy32(plain, act, nz.get().numpy(), want)


# ============================================================================ UAM actor (aac_uam_actor)
_uam = {}


def _uam_model():
    from multi_agent_aac_amd import uam
    from multi_agent_aac_amd import uam_learner as L
    if not _uam:
        _uam["m"] = L.MADDPG([7, 20, 18, 6], [7, 20, 18, 6], 2, n_agents=5, device=DEV, seed=1, batch_size=64,
                             memory_length=4096)
        lib = uam.lib()
        lib.aac_uam_actor_set_tiles.argtypes = [ctypes.c_int32]
        _uam["lib"] = lib
    return _uam["m"], _uam["lib"]


@pytest.fixture(scope="module", autouse=True)
def _drop_uam():
    yield
    if "lib" in _uam:
        _uam["lib"].aac_uam_actor_set_tiles(4)
    _uam.clear()


def _uam_inputs(R, N):
    g = torch.Generator().manual_seed(R)
    own = (torch.rand(R // N, N, 7, dtype=torch.float64, generator=g) * 2 - 1).to(DEV)
    radar = (torch.rand(R // N, N, 18, dtype=torch.float64, generator=g) * 5).to(DEV)
    ep = _episodes(R // N, 12000, R)
    return own, radar, ep


def _uam_case(m, lib, nt, R, N, inputs=None, want_paths=None):
    """Plain and two noisy launches at ``nt`` tiles from counter C0: (plain, noisy 1, noisy 2), each
    checked against the module and the float64 restatement on every row."""
    rpb = 16 * nt
    grid = min((R + rpb - 1) // rpb, CUS)                           # aac_uam_actor: wgs = min(nb, 256)
    p = paths(R, rpb, grid)
    assert p["window"] == NB * grid * rpb
    if want_paths is not None:
        assert (p["fallback_rows"], p["max_kb"], p["wgs_at_max"], p["partial"]) == want_paths
    own, radar, ep = inputs or _uam_inputs(R, N)
    assert lib.aac_uam_actor_set_tiles(nt) == 0
    plain = m.act(own, radar, None, noisy=False)
    ref = m.actors([own.view(-1, 7), radar.view(-1, 18)]).view(R // N, N, 2)
    torch.testing.assert_close(plain, ref, rtol=0, atol=1e-13)
    pl = plain.view(-1, 2).cpu().numpy()
    m.noise_counter.fill_(C0)
    rows = np.arange(R)
    outs = [plain]
    for k in range(2):
        out = m.act(own, radar, ep.to(DEV), noisy=True)
        assert int(m.noise_counter.item()) == C0 + k + 1           # the whole word: arrivals back at 0
        nz = noise_ref.noise64(m.noise_seed, C0 + k, rows, N, ep.numpy(), 10000, 1.0, 0.0)
        np.testing.assert_allclose(out.view(-1, 2).cpu().numpy(), np.clip(pl + nz, -1.0, 1.0), rtol=0, atol=1e-12)
        outs.append(out)
    return outs, p


# tiles = 1: 16 rows per block, window 8 x 256 x 16 = 32 768 rows
UAM_CASES = {
    (32768, 1): (0, 7, 256, False),       # exactly the window
    (32769, 1): (1, 8, 1, True),          # row 32768 alone in block 2048 = index 8 of workgroup 0
    (36907, 13): (4139, 9, 3, True),      # 2307 blocks = 9 x 256 + 3, 11 rows in the last
}


@pytest.mark.parametrize("R,N", list(UAM_CASES))
def test_uam_actor_one_tile_rows_and_noise(native_lib, R, N):
    """uam_actor_ws_kernel<1>, noise-free and noisy: grid = min(ceil(R / 16), 256), window 32 768
    rows.  R = 32 768 is the window; R = 32 769 has one row at block index 8; R = 36 907 = 13 x 2839 has
    2307 blocks (index 8 on every workgroup, index 9 on workgroups 0-2, a last block of 11 rows): 4139
    rows take the inline noise.  There the 2- and 4-tile launches (windows 65 536 and 131 072 rows: every
    row's noise up front) from the same counter value must equal the 1-tile outputs to the bit."""
    m, lib = _uam_model()
    try:
        inputs = _uam_inputs(R, N)
        outs, p = _uam_case(m, lib, 1, R, N, inputs, UAM_CASES[(R, N)])
        if R == 32768:
            assert R == p["window"]
        else:
            assert R > p["window"]
        if R == 36907:
            for nt in (2, 4):
                other, q = _uam_case(m, lib, nt, R, N, inputs)
                assert q["fallback_rows"] == 0 and R < q["window"]
                for a, b in zip(outs, other):
                    assert torch.equal(a, b), nt
    finally:
        lib.aac_uam_actor_set_tiles(4)


def test_uam_actor_default_tiles_past_window(native_lib):
    """The default 4-tile kernel at its own fallback size: 64 rows per block, window 8 x 256 x 64 =
    131 072 rows (the config-5 size).  R = 147 643 = 131 072 + (256 + 3) x 64 - 5: 2307 blocks, block
    index 8 inline on every workgroup, index 9 on workgroups 0-2, 59 rows in the last block: 16 571 rows
    with inline noise.  Module and restatement on every row."""
    m, lib = _uam_model()
    try:
        R = 147643
        assert R == 131072 + (256 + 3) * 64 - 5
        _, p = _uam_case(m, lib, 4, R, 1, want_paths=(R - 131072, 9, 3, True))
        assert p["window"] == 131072 and p["nblk"] == 2307
    finally:
        lib.aac_uam_actor_set_tiles(4)
