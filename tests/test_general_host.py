"""CPU: the flat layout and host-side entry points of the general (any layers list) kernels, csrc/pinn_general.hip."""
import ctypes
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LISTS = [[8, 32, 32, 32, 1], [8, 100, 100, 1], [8, 64, 200, 48, 1], [8, 7, 1, 4, 1], [8, 2000, 300, 1], [8, 256, 256, 256, 1],
         [8, 2048] + [5] * 6 + [4, 1],
         # the lists of test_gpu_regimes.py: one and eight hidden layers, widths beside the 32-wide padding and the 64 x 64 tile edge,
         # kMaxWidth as an output and as an input width
         [8, 33, 65, 7, 1], [8, 130, 1], [8, 40, 24, 72, 8, 96, 31, 64, 36, 1], [8, 2048, 8, 1], [8, 4, 2048, 1]]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from pinn_amd import _lib
    return _lib.load(build_if_missing=False)


@pytest.mark.parametrize("layers", LISTS[:6] + LISTS[7:])
def test_general_offsets_match_oracle_shapes_and_names(layers):
    import pinn_oracle as O
    from pinn_amd import layout
    offs, total = layout.general_offsets(layers)
    params = O.init_params(layers, seed=0)
    names = O.param_names(len(layers) - 2)
    assert [n for n, _, _ in offs] == names
    assert [tuple(s) for _, s, _ in offs] == [tuple(p.shape) for p in params]
    end = 0
    for (_, shape, off), p in zip(offs, params):
        assert off % 4 == 0 and off >= end
        end = off + p.numel()
    assert total == (end + 3) // 4 * 4


def test_general_offsets_equal_fused_layout_for_equal_widths():
    from pinn_amd import layout
    for H, nh in ((256, 3), (128, 1), (1024, 4)):
        assert layout.general_offsets([8] + [H] * nh + [1]) == layout.param_offsets(8, H, nh)
    assert layout.general_offsets([8, 256, 256, 256, 1])[1] == 175362 + 6


@pytest.mark.parametrize("layers", LISTS)
def test_gnet_param_count_matches_python(lib, layers):
    from pinn_amd import _lib, layout
    assert lib.pinn_gnet_param_count(ctypes.byref(_lib.GNet(layers))) == layout.general_offsets(layers)[1]


def test_gnet_rejections(lib):
    from pinn_amd import _lib, layout
    bad = [[8, 0, 32, 1], [8, 32, 3, 1], [8, 2049, 32, 1], [8, 1], [8] + [16] * 9 + [1], [9, 32, 32, 1], [8, 32, 32, 2]]
    for layers in bad:
        with pytest.raises(ValueError):
            layout.check_general(layers)
    for layers in bad[:3] + bad[5:]:
        assert lib.pinn_gnet_param_count(ctypes.byref(_lib.GNet(layers))) == -2, layers
        assert lib.pinn_gnet_workspace_bytes(ctypes.byref(_lib.GNet(layers)), 100, 0) == 0
    g = _lib.GNet([8, 32, 32, 1])
    g.n_hidden = 0
    assert lib.pinn_gnet_param_count(ctypes.byref(g)) == -2
    g.n_hidden = 9
    assert lib.pinn_gnet_param_count(ctypes.byref(g)) == -2
    assert lib.pinn_gnet_param_count(None) == -1


def test_gnet_calls_reject_bad_arguments_without_a_gpu(lib):
    """Argument checks run before anything touches the device."""
    from pinn_amd import _lib
    g = _lib.GNet([8, 100, 100, 1])
    fake = ctypes.c_void_p(1 << 20)
    assert lib.pinn_gnet_forward(ctypes.byref(g), None, fake, 10, None, fake, fake, fake, 1 << 20, None) == -1
    assert lib.pinn_gnet_forward(ctypes.byref(g), fake, fake, 0, None, fake, fake, None, 0, None) == 0       # n_rows == 0
    assert lib.pinn_gnet_forward(ctypes.byref(_lib.GNet([8, 100, 3, 1])), fake, fake, 10, None, fake, fake, fake, 1 << 20, None) == -2
    misaligned = ctypes.c_void_p((1 << 20) + 4)
    assert lib.pinn_gnet_forward(ctypes.byref(g), misaligned, fake, 10, None, fake, fake, fake, 1 << 20, None) == -1
    assert lib.pinn_gnet_forward(ctypes.byref(g), fake, fake, 10, None, fake, fake, fake, 16, None) == -3    # workspace too small
    assert lib.pinn_gnet_mc_dropout(ctypes.byref(g), fake, fake, 10, None, 4, fake, fake, fake, fake, 1 << 20, None) == -1
    assert lib.pinn_gnet_train_grads(ctypes.byref(g), fake, fake, fake, 10, 5, None, fake, fake, fake, 1 << 20, None) == -1
    assert lib.pinn_gnet_train_grads(ctypes.byref(g), fake, fake, fake, 10, 10, None, fake, fake, fake, 16, None) == -3


@pytest.mark.parametrize("layers", LISTS)
def test_gnet_workspace_positive_and_monotone(lib, layers):
    from pinn_amd import _lib
    g = ctypes.byref(_lib.GNet(layers))
    prev = 0
    for n in (1, 15, 17, 1000, 11000, 70000, 1000000):
        b = lib.pinn_gnet_workspace_bytes(g, n, 0)
        assert b > 0 and b >= prev
        prev = b
    assert lib.pinn_gnet_workspace_bytes(g, 1000, 2000) >= lib.pinn_gnet_workspace_bytes(g, 1000, 0)
    assert lib.pinn_gnet_workspace_bytes(g, 1000, 2000) < (4 << 30)
