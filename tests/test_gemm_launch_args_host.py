"""CPU: the packed-row GEMM entry points check their rows descriptor before the first HIP call, all with the same rules and
the same words (csrc/bl_gemm_host.h), then go on to their own rules.  The expected strings are literals, not read from the
code: a change of an error text has to be made here too."""
import ctypes

import pytest

from tests.test_cabi import built_lib  # noqa: F401  (fixture: builds the library when it is missing)

BUF = (ctypes.c_uint8 * 512)()
ALIGNED = (ctypes.addressof(BUF) + 15) & ~15  # every pointer argument; nothing is read through it


def _rows(widths, xp=None):
    from buglab.models import hip_ops

    rows = hip_ops.bl_rows_packed_t()
    rows.nsrc = len(widths)
    for j, w in enumerate(widths[:3]):
        rows.width[j] = w
        rows.xp[j] = ALIGNED if xp is None else xp[j]
    return rows


# how each entry point is called with (rows, M, N, K): every other argument is acceptable, ok=False breaks the entry point's own
# first rule after the descriptor's
def _rows_x6(lib, a, M, N, K, ok=True):
    return lib.bl_gemm_rows_x6(a, None, 0, ALIGNED, 0, None, None, 1, M, N if ok else 30, K, ALIGNED, 32, None)


def _rows_x6_epi(lib, a, M, N, K, ok=True):
    from buglab.models import hip_ops

    return lib.bl_gemm_rows_x6_epi(a, ALIGNED, 0, None, None, 1, M, N if ok else 30, K, None, 0, hip_ops.NO_DROPOUT.c(), ALIGNED, 32, None)


def _rows_x6w(lib, a, M, N, K, ok=True):
    return lib.bl_gemm_rows_x6w(a, None, 0, ALIGNED, 0, None, None, 1, M, 256 if ok else 128, K, ALIGNED, 256, None)


def _wgrad_x6(lib, a, M, N, K, ok=True):
    return lib.bl_gemm_wgrad_x6(a, ALIGNED, None, None, None, 1, M, N if ok else 48, K, ALIGNED, 0, 32, None)


def _wgrad_routed_x6(lib, a, M, N, K, ok=True):
    return lib.bl_gemm_wgrad_routed_x6(a, ALIGNED, ALIGNED, ALIGNED, 1, None, None, 1, M, N if ok else 48, K, ALIGNED, 0, 32, None)


def _rows_h3(lib, a, M, N, K, ok=True):
    return lib.bl_gemm_rows_h3(a, None, 0, ALIGNED, 0, None, None, 1, M, N if ok else 30, K, 1.0, None, ALIGNED, 32, None)


def _wgrad_h3(lib, a, M, N, K, ok=True):
    return lib.bl_gemm_wgrad_h3(a, ALIGNED, None, None, 0, None, None, 1, M, N, K, 1.0 if ok else 0.0, None, ALIGNED, 0, 32, None)


ENTRY_POINTS = {
    "bl_gemm_rows_x6": (_rows_x6, "bl_gemm_rows_x6: N/ldc multiples of 4, aligned pointers required"),
    "bl_gemm_rows_x6_epi": (_rows_x6_epi, "bl_gemm_rows_x6_epi: N/ldc multiples of 4, aligned pointers required"),
    "bl_gemm_rows_x6w": (_rows_x6w, "bl_gemm_rows_x6w: N must be a multiple of 256 and K of 64 (bl_gemm_rows_x6w_ok)"),
    "bl_gemm_wgrad_x6": (_wgrad_x6, "bl_gemm_wgrad_x6: N a multiple of 32 and aligned pointers required"),
    "bl_gemm_wgrad_routed_x6": (_wgrad_routed_x6, "bl_gemm_wgrad_routed_x6: N a multiple of 32 and aligned pointers required"),
    "bl_gemm_rows_h3": (_rows_h3, "bl_gemm_rows_h3: N/ldc multiples of 4, aligned pointers required"),
    "bl_gemm_wgrad_h3": (_wgrad_h3, "bl_gemm_wgrad_h3: N a multiple of 32, aligned pointers and a positive out_scale required"),
}

# (widths, source pointers or None for aligned ones, K, the message after "<entry point>: ")
BAD_DESCRIPTORS = {
    "nsrc=0": ([], None, 64, "rows descriptor needs 1..3 sources"),
    "nsrc=4": ([32, 32, 32, 32], None, 128, "rows descriptor needs 1..3 sources"),
    "null source": ([32, 32], [ALIGNED, None], 64, "source 1: packed pointer 16-byte aligned and width a multiple of 32 required"),
    "pointer off by 2": ([64], [ALIGNED + 2], 64, "source 0: packed pointer 16-byte aligned and width a multiple of 32 required"),
    "width=48": ([48], None, 48, "source 0: packed pointer 16-byte aligned and width a multiple of 32 required"),
    "32+64 is not K=128": ([32, 64], None, 128, "K (128) != sum of source widths (96)"),
}


@pytest.fixture(scope="module")
def lib(built_lib):  # noqa: F811
    from buglab.models import hip_ops

    return hip_ops.load_library()


@pytest.mark.parametrize("case", list(BAD_DESCRIPTORS))
@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_bad_rows_descriptor_is_reported_in_the_shared_words(lib, name, case):
    widths, xp, K, message = BAD_DESCRIPTORS[case]
    rc = ENTRY_POINTS[name][0](lib, ctypes.byref(_rows(widths, xp)), 8, 64, K)
    assert rc != 0
    assert lib.bl_last_error().decode() == f"{name}: {message}"


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_own_rules_follow_the_descriptor_rules(lib, name):
    call, own_message = ENTRY_POINTS[name]
    good = _rows([64])
    assert call(lib, ctypes.byref(good), 8, 64, 64, ok=False) != 0
    assert lib.bl_last_error().decode() == own_message
    # both broken: the descriptor is reported, it is checked first
    assert call(lib, ctypes.byref(_rows([48])), 8, 64, 48, ok=False) != 0
    assert lib.bl_last_error().decode() == f"{name}: source 0: packed pointer 16-byte aligned and width a multiple of 32 required"


@pytest.mark.parametrize("name", list(ENTRY_POINTS))
def test_no_rows_is_ok_before_any_check(lib, name):
    assert ENTRY_POINTS[name][0](lib, ctypes.byref(_rows([])), 0, 64, 64) == 0
    assert ENTRY_POINTS[name][0](lib, None, 0, 64, 64) == 0


def test_row_packers_name_themselves(lib):
    assert lib.bl_pack_bf16x3(None, 64, 4, 64, ALIGNED, None) != 0
    assert lib.bl_last_error().decode() == "bl_pack_bf16x3: null or misaligned pointer"
    assert lib.bl_pack_bf16x3(ALIGNED, 64, 4, 12, ALIGNED + 2, None) != 0
    assert lib.bl_last_error().decode() == "bl_pack_bf16x3: null or misaligned pointer"
    assert lib.bl_pack_bf16x3(ALIGNED, 64, 4, 12, ALIGNED, None) != 0
    assert lib.bl_last_error().decode() == "bl_pack_bf16x3: D must be a multiple of 8 (got 12)"
    assert lib.bl_pack_bf16x3(ALIGNED, 62, 4, 64, ALIGNED, None) != 0
    assert lib.bl_last_error().decode() == "bl_pack_bf16x3: D must be a multiple of 8 (got 64)"
    assert lib.bl_pack_bf16x3_cols(ALIGNED, 64, 4, 64, 128, 64, None, None) != 0
    assert lib.bl_last_error().decode() == "bl_pack_bf16x3_cols: null or misaligned pointer"
    for D, D_total, col_off in ((12, 128, 0), (64, 128, 72), (64, 128, 4), (64, 100, 0), (64, 128, -8)):
        assert lib.bl_pack_bf16x3_cols(ALIGNED, 64, 4, D, D_total, col_off, ALIGNED, None) != 0
        assert lib.bl_last_error().decode() == "bl_pack_bf16x3_cols: widths / offset must be multiples of 8 with col_off + D <= D_total"
    assert lib.bl_pack_bf16x3(None, 64, 0, 12, None, None) == 0
    assert lib.bl_pack_bf16x3_cols(None, 64, 0, 12, 8, 4, None, None) == 0
