"""The learner monitor's host side (no GPU): ``read()``'s ring unwrapping and field table on synthetic
buffers, and the field-name table against include/aac_monitor.h."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "aac_monitor.h")) as f:
        return f.read()


def _define(text, name):
    return int(re.search(rf"#define {name} (\d+)", text).group(1))


def test_field_table_matches_header():
    from multi_agent_aac_amd import monitor
    h = _header()
    assert monitor.FIELDS == _define(h, "AAC_MONITOR_FIELDS") == len(monitor.FIELD_NAMES)
    assert monitor.VEC_WG == _define(h, "AAC_MONITOR_VEC_WG")
    assert monitor.VEC_VALUES == _define(h, "AAC_MONITOR_VEC_VALUES")
    assert monitor.MAX_COLS == _define(h, "AAC_MONITOR_MAX_COLS")
    assert len(monitor.NETS) == _define(h, "AAC_MONITOR_NETS") and len(monitor.AGG) == _define(h, "AAC_MONITOR_AGG")
    # the documented field order: "<index> <name>" pairs of the header's table
    table = h[h.index("Field order"):h.index("The sums of squares")]
    pairs = {int(i): n for i, n in re.findall(r"(?<![\w.])(\d+) ([a-z][a-z_]*[a-z])", table)}
    assert pairs == dict(enumerate(monitor.FIELD_NAMES))
    assert monitor.FIELD_NAMES.index("rows_nonfinite") == _define(h, "AAC_MONITOR_F_ROWS_NONFINITE")
    assert monitor.FIELD_NAMES.index("critic_grad_sumsq") == _define(h, "AAC_MONITOR_F_NET0")
    assert [monitor.FIELD_NAMES[i] for i in monitor.COUNT_FIELDS] == [
        "rows_nonfinite", "critic_grad_nonfinite", "critic_param_nonfinite", "actor_grad_nonfinite",
        "actor_param_nonfinite"]


def _synthetic(counter, R, A):
    """Buffers as ``counter`` commits would leave them: record u holds u + c / 10 + f / 1000."""
    from multi_agent_aac_amd import monitor
    F = monitor.FIELDS
    ring, upd = np.zeros((R, A, F)), np.full(R, -1, dtype=np.int64)
    value = lambda u: u + np.arange(A)[:, None] / 10 + np.arange(F)[None, :] / 1000   # noqa: E731
    agg = np.zeros((5, A, F))
    agg[3], agg[4] = np.inf, -np.inf
    for u in range(counter):
        ring[u % R], upd[u % R] = value(u), u
        v = value(u)
        agg[0] += 1
        agg[1] += v
        agg[2] += v * v
        agg[3], agg[4] = np.minimum(agg[3], v), np.maximum(agg[4], v)
    return ring, upd, agg, value


@pytest.mark.parametrize("counter", [0, 3, 4, 5, 6, 23])       # below R, equal to R, above R, wrapped several times
@pytest.mark.parametrize("A", [1, 3])
def test_read_unwraps_the_ring(counter, A):
    from multi_agent_aac_amd import monitor
    R = 4
    ring, upd, agg, value = _synthetic(counter, R, A)
    out = monitor.unwrap(counter, ring, upd, agg, -1)
    n = min(counter, R)
    assert out["updates"] == counter and out["bad_update"] == -1
    assert out["update"].dtype == np.int64
    np.testing.assert_array_equal(out["update"], np.arange(counter - n, counter))
    for f, name in enumerate(monitor.FIELD_NAMES):
        assert out[name].shape == (n, A)
        want = np.array([value(u)[:, f] for u in range(counter - n, counter)]).reshape(n, A)
        np.testing.assert_array_equal(out[name], want)
    # norms are square roots taken on the host
    for net in monitor.NETS:
        np.testing.assert_array_equal(out[f"grad_norm_{net}"], np.sqrt(out[f"{net}_grad_sumsq"]))
        np.testing.assert_array_equal(out[f"param_norm_{net}"], np.sqrt(out[f"{net}_param_sumsq"]))
    # aggregates over every update since the reset, not only the kept ones
    for f, name in enumerate(monitor.FIELD_NAMES):
        if counter == 0:
            assert np.isnan(out["mean"][name]).all() and np.isnan(out["min"][name]).all()
            continue
        vals = np.array([value(u)[:, f] for u in range(counter)])
        np.testing.assert_allclose(out["mean"][name], vals.mean(axis=0), rtol=1e-12)
        np.testing.assert_allclose(out["std"][name], vals.std(axis=0), atol=1e-6)
        np.testing.assert_array_equal(out["min"][name], vals.min(axis=0))
        np.testing.assert_array_equal(out["max"][name], vals.max(axis=0))
        np.testing.assert_array_equal(out["count"][name], np.full(A, counter))


def test_restatement_orders_differ_only_in_rounding():
    """The two copy orders of the restatement are the documented ones (a fixed float32 example)."""
    import monitor_ref
    g = np.array([[1.0], [2.0 ** -24], [2.0 ** -24], [2.0 ** -24]], dtype=np.float32)
    # in sequence every 2^-24 is rounded away; grouped, (g2 + g3) = 2^-23 survives
    assert monitor_ref.sum_copies(g, 0)[0] == np.float32(1.0)
    assert monitor_ref.sum_copies(g, 1)[0] == np.float32(1.0) + np.float32(2.0 ** -23)
