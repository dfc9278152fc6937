"""CPU-only checks of the value-baseline fit's C ABI (amx_vfit_work, amx_vfit_param_count,
amx_vfit_epoch): sizes are pure host arithmetic, and bad arguments are refused with
AMX_E_INVAL and a message naming the entry point before anything touches a GPU."""
import ctypes

import pytest

from amp_extensions_amd import _build, _native


@pytest.fixture(scope="module")
def lib():
    path = _build.build(verbose=False)
    return _native.load(path)


def epoch(lib, ctx=None, n_rows=128, perm=8, kf=256, H0p=128, H1p=128):
    """amx_vfit_epoch with every pointer a non-null dummy unless overridden: each call here must
    be refused by the argument checks, which never dereference anything."""
    d = ctypes.c_void_p(4096)
    return lib.amx_vfit_epoch(ctx, n_rows, d, kf, d, ctypes.c_void_p(perm) if perm else None, kf, H0p, H1p,
                              d, d, d, d, d, d, d, d, d, 1e-3, 0.9, 0.999, 1e-8, 1e-3, d, d, None)


def test_workspace_and_parameter_counts_are_host_arithmetic(lib):
    # h0, h1, dz1, dz0 [128, 64] each, gW1 [128, 128], head partials [8, 64], y, dy [64], 64 header floats
    # plus the gathered batch [64, kf]
    floats = 64 + 4 * 128 * 64 + 128 * 128 + 8 * 64 + 2 * 64
    assert lib.amx_vfit_work(256, 128, 128) == 4 * (floats + 64 * 256)
    assert lib.amx_vfit_work(224, 128, 128) == 4 * (floats + 64 * 224)
    # W0 | b0 | W1 | b1 | w2 | b2
    assert lib.amx_vfit_param_count(256, 128, 128) == 128 * 256 + 128 + 128 * 128 + 128 + 128 + 1
    assert lib.amx_vfit_param_count(224, 128, 128) == 128 * 224 + 128 + 128 * 128 + 128 + 128 + 1
    for bad in ((230, 128, 128), (0, 128, 128), (256, 256, 128), (256, 128, 64)):
        assert lib.amx_vfit_work(*bad) == -1
        assert b"amx_vfit_work" in lib.amx_last_error()
        assert lib.amx_vfit_param_count(*bad) == -1
        assert b"amx_vfit_param_count" in lib.amx_last_error()


def test_epoch_refuses_null_context(lib):
    assert epoch(lib, ctx=None) == -1
    assert b"amx_vfit_epoch" in lib.amx_last_error() and b"null ctx" in lib.amx_last_error()


def test_epoch_checks_come_before_the_gpu(lib):
    """With a context the remaining checks run in order; a fake (never dereferenced beyond
    its S field) context is enough because every case is refused before a launch."""
    fake = (ctypes.c_int * 512)()  # zeroed amx_ctx stand-in: S = 0
    ctx = ctypes.cast(fake, ctypes.c_void_p)
    assert epoch(lib, ctx=ctx, n_rows=127) == -1
    assert b"amx_vfit_epoch" in lib.amx_last_error() and b"n_rows=127" in lib.amx_last_error()
    assert epoch(lib, ctx=ctx, perm=0) == -1
    assert b"amx_vfit_epoch" in lib.amx_last_error() and b"perm" in lib.amx_last_error()
    assert epoch(lib, ctx=ctx, kf=230) == -1
    assert b"amx_vfit_epoch" in lib.amx_last_error() and b"kf=230" in lib.amx_last_error()
    assert epoch(lib, ctx=ctx, H0p=256) == -1
    assert b"amx_vfit_epoch" in lib.amx_last_error() and b"hidden" in lib.amx_last_error()


def test_python_refusals_need_no_gpu():
    """DeviceMLPBaseline.fit's shape refusals are decided from host-side fields alone."""
    from amp_extensions_amd.gae import DeviceMLPBaseline
    bl = DeviceMLPBaseline.__new__(DeviceMLPBaseline)
    bl.widths, bl.batch_size = [128, 128], 64
    assert bl.fit_supported()
    for widths, batch in (([128, 128], 32), ([128, 128, 128], 64), ([256, 128], 64), ([128], 64)):
        bl.widths, bl.batch_size = widths, batch
        assert not bl.fit_supported()
        with pytest.raises(NotImplementedError):
            bl.fit([])
