"""CPU: the guard-band helper of the C-ABI stride tests (tests/guard_bands.py) -- its geometry, that assert_untouched trips on
a single flipped bit anywhere outside the payload and names the place, and that payload writes never trip it.  Also the argument
checks the strided entry points make on the host (return code only: no launch, no GPU)."""
import ctypes
import os

import pytest
import torch

from tests.conftest import PKG
from tests.guard_bands import PATTERN_16, PATTERN_32, guarded

LIB = os.path.join(PKG, "buglab", "models", "hip_ops", "libbuglab_hip.so")


@pytest.mark.parametrize("dtype,width,ld", [(torch.float32, 96, 100), (torch.float32, 8, 44), (torch.int32, 160, 196), (torch.int16, 288, 296),
                                            (torch.int16, 64, 136), (torch.int8, 6, 16)])
def test_geometry(dtype, width, ld):
    rows = 5
    g = guarded(rows, width, ld=ld, dtype=dtype, device="cpu")
    item = torch.empty((), dtype=dtype).element_size()
    assert g.ld == ld and (ld * item) % 16 == 0
    assert g.view.shape == (rows, width) and g.view.stride() == (ld, 1) and g.view.dtype == dtype
    # 16-byte aligned as the ABI asks, and deliberately not better: lead = 4 floats
    assert g.view.data_ptr() % 16 == 0 and g.view.data_ptr() % 32 == 16
    assert g.view.data_ptr() - g.bits.data_ptr() == (256 * ld) * item + 16
    assert g.bits.numel() * item == (2 * 256 * ld + rows * ld) * item + 16
    # every element starts as the pattern: NaN as a float, the payload included
    if dtype == torch.float32:
        assert torch.isnan(g.bits.view(torch.float32)).all() and int(g.bits[0]) == PATTERN_32
    if dtype == torch.int16:
        assert int(g.bits[0]) == PATTERN_16
        assert torch.isnan(g.bits.view(torch.bfloat16).float()).all() and torch.isnan(g.bits.view(torch.float16).float()).all()
    g.assert_untouched("fresh")
    # payload round trip through the strided view; the flat allocation holds it at offset + r * ld + c
    want = (torch.arange(rows * width).reshape(rows, width) % 100).to(dtype)
    g.fill(want)
    assert torch.equal(g.view, want) and torch.equal(g.payload(), want) and g.payload().is_contiguous()
    assert g.bits.view(dtype)[g.offset + 3 * ld + (width - 1)] == want[3, width - 1]
    g.assert_untouched("after payload writes")
    g.view.zero_()
    g.view[rows - 1, width - 1] = 1
    g.assert_untouched("after more payload writes")


def test_lead_zero_is_aligned_like_the_allocator():
    g = guarded(3, 8, ld=8, dtype=torch.float32, device="cpu", lead=0, guard_rows=2)
    assert g.view.data_ptr() % 32 == 0 and g.view.is_contiguous() and g.bits.numel() == (2 + 3 + 2) * 8


@pytest.mark.parametrize("dtype", [torch.float32, torch.int16])
@pytest.mark.parametrize("where", ["just before the payload", "padding column", "row after the payload", "last guard element", "first element"])
def test_a_single_bit_flip_outside_the_payload_is_found_and_named(dtype, where):
    rows, width, ld = 7, 24, 32
    g = guarded(rows, width, ld=ld, dtype=dtype, device="cpu")
    g.fill(1)
    flat, text = {
        "just before the payload": (g.offset - 1, f"row -1, col {ld - 1}"),
        "padding column": (g.offset + 2 * ld + width, f"row 2, col {width}"),
        "row after the payload": (g.offset + rows * ld + 3, "row M+0, col 3"),
        "last guard element": (g.bits.numel() - 1, f"row M+255, col {ld - 1}"),
        "first element": (0, "row -257, "),
    }[where]
    g.bits[flat] ^= 1
    with pytest.raises(AssertionError) as e:
        g.assert_untouched("planted")
    assert "planted" in str(e.value) and text in str(e.value) and "1 element(s)" in str(e.value), str(e.value)
    g.bits[flat] ^= 1
    g.assert_untouched("restored")


def test_the_gap_between_groups_is_guard():
    """a grouped weight gradient: gw_group_stride = (K + 3) * ld_gw -- the three rows between two groups belong to the guard"""
    K, N, ld, T = 5, 8, 12, 3
    live = (torch.arange(T * (K + 3)) % (K + 3)) < K
    g = guarded(T * (K + 3), N, ld=ld, dtype=torch.float32, device="cpu", live_rows=live)
    g.fill(0.5)
    assert g.payload().shape == (T * K, N) and bool((g.payload() == 0.5).all())
    assert torch.isnan(g.view[K]).all()  # a gap row kept the pattern
    g.assert_untouched("filled")
    g.view[K + 3, 2] = 7.0   # first row of group 1: payload
    g.assert_untouched("payload write")
    g.view[K + 1, 2] = 7.0   # gap row
    with pytest.raises(AssertionError, match=f"row {K + 1}, col 2"):
        g.assert_untouched("gap write")


def test_bad_geometry_is_refused():
    with pytest.raises(ValueError):
        guarded(4, 8, ld=10, dtype=torch.float32, device="cpu")  # ld not a multiple of 4 floats
    with pytest.raises(ValueError):
        guarded(4, 8, ld=4, dtype=torch.float32, device="cpu")   # ld < width
    with pytest.raises(ValueError):
        guarded(4, 8, ld=12, dtype=torch.int16, device="cpu")    # 24-byte rows


def test_strided_entry_points_refuse_a_leading_dimension_below_the_width():
    """bl_segment_max_fwd, bl_gru_cell_* and bl_mp_scatter_grad* address x + row * ld with scalar loads: any D and ld work (the
    heads call the segmented max with D = 1), but an ld below the width makes rows overlap -- refused on the host, before any HIP
    call (these checks precede the launch in csrc/bl_graph_ops.hip), with BL_EINVAL and a message."""
    if not os.path.exists(LIB):
        import __graft_entry__ as g

        g.build()
    from buglab.models import hip_ops

    lib = hip_ops.load_library()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    nodrop = hip_ops.Dropout(0.0, 0, 0).c()
    EINVAL = -1
    rc = lib.bl_segment_max_fwd(p, 4, p, None, 2, 8, 0, p, None, None, None, 1e-5, None, None, None, None, None, None, None)
    assert rc == EINVAL and b"ldx" in lib.bl_last_error()
    rc = lib.bl_gru_cell_fwd(p, p, p, 4, 2, 8, nodrop, p, None)
    assert rc == EINVAL and b"ld_h" in lib.bl_last_error()
    rc = lib.bl_gru_cell_bwd(p, p, p, p, 4, 2, 8, nodrop, p, p, p, None)
    assert rc == EINVAL and b"ld_h" in lib.bl_last_error()
    rc = lib.bl_mp_scatter_grad(p, 16, p, p, p, p, 2, 8, 0, p, 4, None, None)
    assert rc == EINVAL and b"ld_gh" in lib.bl_last_error()
    rc = lib.bl_mp_scatter_grad(p, 12, p, p, p, p, 2, 8, 0, p, 8, None, None)  # (the check that was there: ld_ga < 2 Din)
    assert rc == EINVAL
    rc = lib.bl_mp_scatter_grad_split(p, 16, p, p, p, p, 2, 8, 4, p, 2, p, 4, None, None)
    assert rc == EINVAL
