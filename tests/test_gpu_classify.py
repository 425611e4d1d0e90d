"""GPU: the end of a decision that both SVC kernels share (csrc/pinn_ovo.h: votes, the first maximum, a row that reads nothing)
through `_decide` of DeviceLinearSVC and DeviceKernelSVC, backend="device" against backend="host" of the same hand-made model
(tests/test_classify_host.py: every sign is exact, ties and exactly-zero values are present).

Gates: votes and predictions equal element for element; the linear model's values bit for bit (they are sums of -1, 0 and +1);
the kernel model's values within 1e-12 x the absolute term K of their only term, so an exact zero stays one.
2, 3 and 8 classes: one pair, the cycle, all 28 pairs; 1, 127 and 129 rows: either side of both kernels' 128-row tile."""
import numpy as np
import pytest

from test_classify_host import CLASSES, KINDS, ROWS, drawn_rows, hand_model, ties_and_zeros

pytestmark = pytest.mark.gpu
WANT = ("decision", "votes", "pred")


def both(m, X, **kw):
    m.backend = "host"
    h = m._decide(X, want=WANT, **kw)
    m.backend = "device"
    return h, m._decide(X, want=WANT, **kw)


def check_equal(kind, h, d, what):
    err = np.abs(d["decision"] - h["decision"])
    print("%s: %d rows, largest difference of a value %.3e" % (what, len(err), err.max()))
    assert d["votes"].dtype == d["pred"].dtype == np.int64 and d["decision"].dtype == np.float64
    assert np.array_equal(d["votes"], h["votes"]) and np.array_equal(d["pred"], h["pred"])
    if kind == "linear":
        assert d["decision"].tobytes() == h["decision"].tobytes()
    else:
        assert (err <= 1e-12 * np.abs(h["decision"])).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("C", CLASSES)
def test_shared_epilogue_against_the_host(kind, C):
    m, rng = hand_model(kind, C)
    for n in ROWS:
        h, d = both(m, drawn_rows(rng, n))
        tie, zero = ties_and_zeros(h)
        assert n == 1 or ((np.abs(h["decision"]) > 0.0).any() and (C == 2 or (zero.any() and tie.any())))
        check_equal(kind, h, d, "%s, %d classes" % (kind, C))


@pytest.mark.parametrize("kind", KINDS)
def test_a_row_index_outside_the_array_reads_nothing(kind):
    m, rng = hand_model(kind, 3)
    X = drawn_rows(rng, 140)
    idx = rng.integers(0, 140, 129)
    bad = idx.copy()
    bad[[5, 128]] = 140, -1                              # just past the end, and before the start
    ok = np.ones(129, dtype=bool)
    ok[[5, 128]] = False
    h, _ = both(m, X, row_index=idx)
    m.backend = "device"
    d = m._decide(X, row_index=bad, want=WANT)
    assert np.isnan(d["decision"][~ok]).all() and (d["votes"][~ok] == 0).all() and (d["pred"][~ok] == -1).all()
    check_equal(kind, {k: v[ok] for k, v in h.items()}, {k: v[ok] for k, v in d.items()}, "%s, gathered rows" % kind)
