"""CPU: the pinn_lr_batch_* entry points of include/pinn_hip.h with the library built and no device.  Every refusal is
decided on the host before any launch, so the addresses handed over are never dereferenced; the size functions return 0
outside the limits and a workspace that grows with the rows, not with the cap of 1024 partials."""
import ctypes

import pytest

E_ARG, E_WS = -1, -3
ONE = 0x1000                               # a non-NULL, aligned address that no call below may touch


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def head(n_batch=2, n_feat=(1, 2), cols=(0, 0, 3, 4), max_feat=2, ld=22, n=100, n_classes=2, d_arr=ONE, d_y=ONE, d_n_feat=ONE, d_cols=ONE):
    return (d_arr, ld, 1000, None, n, d_y, n_classes, n_batch, ints(*n_feat), ints(*cols), max_feat, d_n_feat, d_cols)


def entry_points(lib):
    big = 1 << 40
    return {
        "scaler": lambda h, ws=big, st=ONE: lib.pinn_lr_batch_scaler(*h, 1, st, ONE, ws, None),
        "newton": lambda h, ws=big, st=ONE: lib.pinn_lr_batch_newton(*h, 4, 1e-4, 1.0, 1, st, ONE, ws, None),
        "score": lambda h, ws=big, st=ONE: lib.pinn_lr_batch_score(*h, st, 0, ONE, ONE, None, ONE, ws, None),
    }


def test_constants_agree_with_the_header():
    import os
    import re
    from pinn_amd import _lib, featsel
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pinn_hip.h")).read()
    assert int(re.search(r"#define PINN_LR_MAX_BATCH (\d+)", text).group(1)) == 4096 == _lib.LR_MAX_BATCH == featsel.MAX_BATCH
    for name in ("SINGULAR", "NAN", "STALLED"):
        assert int(re.search(r"#define PINN_LR_%s (\d+)" % name, text).group(1)) == getattr(featsel, name)
    for name in ("scaler", "newton", "score", "auc", "state_stride", "workspace_bytes"):
        assert "pinn_lr_batch_" + name in _lib.declared_symbols()


def test_sizes(lib):
    assert lib.pinn_lr_batch_state_stride(2, 8) >= lib.pinn_lr_state_bytes(2, 8) > 0
    assert lib.pinn_lr_batch_state_stride(5, 3) % 256 == 0 and lib.pinn_lr_batch_state_stride(13, 4) >= lib.pinn_lr_state_bytes(13, 4)
    for C, D in ((1, 2), (14, 2), (2, 0), (2, 9), (13, 5), (8, 8)):
        assert lib.pinn_lr_batch_state_stride(C, D) == 0 and lib.pinn_lr_batch_workspace_bytes(1000, 4, C, D) == 0, (C, D)
    assert lib.pinn_lr_batch_workspace_bytes(1000, 0, 2, 3) == 0 and lib.pinn_lr_batch_workspace_bytes(1000, 4097, 2, 3) == 0
    assert lib.pinn_lr_batch_workspace_bytes(-1, 4, 2, 3) == 0
    one = lib.pinn_lr_batch_workspace_bytes(1300, 1, 2, 4)
    assert lib.pinn_lr_batch_workspace_bytes(1300, 4096, 2, 4) == 4096 * one
    # the partials of a candidate: row_blocks(n, 128, 1024) slots, so 4096 candidates at 1.3e3 rows stay small
    small, large = lib.pinn_lr_batch_workspace_bytes(1300, 4096, 2, 4), lib.pinn_lr_batch_workspace_bytes(131072 + 5, 4096, 2, 4)
    print("4096 candidates, C = 2, D <= 4: %.1f MiB at 1.3e3 rows, %.1f MiB at 1.3e5; one single model: %.1f MiB" %
          (small / 2 ** 20, large / 2 ** 20, lib.pinn_lr_workspace_bytes(1300, 2, 4) / 2 ** 20))
    n_sums = 1 + 2 * 5 + 3 * 15
    assert small <= 4096 * (11 * (n_sums + 13) * 8 + n_sums * 8 + 3 * 256) and small < 64 << 20
    assert large == lib.pinn_lr_batch_workspace_bytes(10 ** 7, 4096, 2, 4)                  # the cap of 1024 partials
    assert lib.pinn_lr_batch_workspace_bytes(129, 1, 2, 4) > lib.pinn_lr_batch_workspace_bytes(128, 1, 2, 4)      # two tiles, two partials


def test_refusals_come_before_any_launch(lib):
    for name, f in entry_points(lib).items():
        assert f(head(n_batch=0)) == E_ARG, name
        assert f(head(n_batch=4097)) == E_ARG, name
        assert f(head(n_feat=(0, 2))) == E_ARG, name                                 # n_feat[c] below 1
        assert f(head(n_feat=(1, 3))) == E_ARG, name                                 # above max_feat
        assert f(head(cols=(0, 0, 3, 22))) == E_ARG, name                            # a column at ld
        assert f(head(cols=(-1, 0, 3, 4))) == E_ARG, name
        assert f(head(n_classes=13, max_feat=5, n_feat=(1, 2), cols=(0,) * 10)) == E_ARG, name      # outside in_limits
        assert f(head(n_classes=1)) == E_ARG and f(head(max_feat=9, cols=(0,) * 18)) == E_ARG, name
        assert f(head(n=0)) == E_ARG and f(head(ld=0)) == E_ARG, name
        assert f(head(d_arr=None)) == E_ARG and f(head(d_y=None)) == E_ARG, name
        assert f(head(d_n_feat=None)) == E_ARG and f(head(d_cols=None)) == E_ARG, name
        assert f(head(d_arr=ONE + 4)) == E_ARG, name                                 # alignment
        assert f(head(), st=None) == E_ARG, name
        need = lib.pinn_lr_batch_workspace_bytes(100, 2, 2, 2)
        assert need > 0 and f(head(), ws=need - 1) == E_WS and f(head(), ws=0) == E_WS, name
    h = head()
    assert lib.pinn_lr_batch_scaler(*h, 1, ONE, None, 1 << 40, None) == E_ARG            # no workspace
    assert lib.pinn_lr_batch_newton(*h, -1, 1e-4, 1.0, 1, ONE, ONE, 1 << 40, None) == E_ARG
    assert lib.pinn_lr_batch_newton(*h, 4, -1.0, 1.0, 1, ONE, ONE, 1 << 40, None) == E_ARG
    assert lib.pinn_lr_batch_newton(*h, 4, 1e-4, 0.0, 1, ONE, ONE, 1 << 40, None) == E_ARG
    assert lib.pinn_lr_batch_score(*h, ONE, 2, ONE, ONE, None, ONE, 1 << 40, None) == E_ARG       # normal_class outside the classes
    assert lib.pinn_lr_batch_score(*h, ONE, 0, None, ONE, None, ONE, 1 << 40, None) == E_ARG
    assert lib.pinn_lr_batch_score(*h, ONE, 0, ONE, None, None, ONE, 1 << 40, None) == E_ARG
    for args in ((None, ONE, 10, 2, ONE), (ONE, None, 10, 2, ONE), (ONE, ONE, 10, 2, None), (ONE, ONE, 0, 2, ONE), (ONE, ONE, 10, 0, ONE),
                 (ONE, ONE, 10, 4097, ONE), (ONE + 4, ONE, 10, 2, ONE)):
        assert lib.pinn_lr_batch_auc(*args, None) == E_ARG, args
