"""The Float32 solver's route (csrc/ins_f32.hip: ins_f32_choose) without a device: the choice for an all-periodic uniform box under the switches that
select it, written out from the conditions ins_poisson_spectral_create_f32 had before the route was a value of its own:

    float2 spectra : 3-D, INS_F32_HIPFFT_PROJECT off, the fp64 solver of the box runs on own passes (all three sides 2^m in 16 .. 1024 or, without
                     INS_OWNFFT_POW2_ONLY, one of 96 192 384 160 320 640; INS_DISABLE_OWNFFT and INS_DISABLE_ZSOLVE off), the z side one of
                     192 256 384 512 and INS_F32_FP64_SPECTRA off
    fp64 spectra   : the same without the last two conditions
    hipFFT         : everything else

INS_F32_SPLIT_GRADIENT is read per projection and moves no route."""
import pytest

# F32Route of csrc/ins_f32_internal.h; SpectralRoute of csrc/ins_internal.h from ROUTE_OWN2D on is an own route
HIPFFT, FP64_SPECTRA, FLOAT2_SPECTRA, WRAP = range(4)
ROUTE_OWN2D = 2

# (box, switches, route)
TABLE = [
    ((32, 32), {}, HIPFFT),  # 2-D boxes have no fp64 passes fed from a float field
    ((24, 18), {}, HIPFFT),
    ((64, 256), {}, HIPFFT),
    ((66, 12, 10), {}, HIPFFT),
    ((128, 16, 16), {}, FP64_SPECTRA),
    ((32, 16, 16), {}, FP64_SPECTRA),
    ((128, 16, 256), {}, FLOAT2_SPECTRA),
    ((256, 16, 192), {}, FLOAT2_SPECTRA),
    ((32, 16, 512), {}, FLOAT2_SPECTRA),
    ((32, 16, 384), {}, FLOAT2_SPECTRA),
    ((32, 16, 128), {}, FP64_SPECTRA),  # a z side of the fp64 z kernel that the float2 one does not have
    ((32, 16, 1024), {}, FP64_SPECTRA),
    ((24, 20, 256), {}, HIPFFT),  # z sides of the float2 kernel under x / y sides without own passes
    ((48, 16, 384), {}, HIPFFT),
    ((128, 20, 192), {}, HIPFFT),
    ((66, 16, 512), {}, HIPFFT),
    ((128, 16, 256), dict(INS_F32_FP64_SPECTRA=1), FP64_SPECTRA),
    ((128, 16, 256), dict(INS_F32_HIPFFT_PROJECT=1), HIPFFT),
    ((128, 16, 256), dict(INS_F32_HIPFFT_PROJECT=1, INS_F32_FP64_SPECTRA=1), HIPFFT),
    ((128, 16, 256), dict(INS_F32_SPLIT_GRADIENT=1), FLOAT2_SPECTRA),
    ((128, 16, 16), dict(INS_F32_SPLIT_GRADIENT=1), FP64_SPECTRA),
    ((128, 16, 16), dict(INS_F32_FP64_SPECTRA=1), FP64_SPECTRA),
    ((128, 16, 16), dict(INS_F32_HIPFFT_PROJECT=1), HIPFFT),
    ((128, 16, 256), dict(INS_DISABLE_OWNFFT=1), HIPFFT),
    ((32, 16, 16), dict(INS_DISABLE_OWNFFT=1), HIPFFT),
    ((128, 16, 256), dict(INS_DISABLE_ZSOLVE=1), HIPFFT),  # the own passes end in the fused z kernel: without it the fp64 solver is on rocFFT
    ((128, 16, 16), dict(INS_DISABLE_ZSOLVE=1), HIPFFT),
    ((256, 16, 192), dict(INS_OWNFFT_POW2_ONLY=1), HIPFFT),
    ((128, 16, 256), dict(INS_OWNFFT_POW2_ONLY=1), FLOAT2_SPECTRA),
    ((32, 32), dict(INS_F32_FP64_SPECTRA=1), HIPFFT),
]


@pytest.mark.parametrize("n,opts,route", TABLE)
def test_route_chosen_for_a_box(n, opts, route):
    from ins_amd import _lib

    lib = _lib.load()
    n3 = tuple(n) + (1,) * (3 - len(n))
    with _lib.options(**opts):
        got = lib.ins_dbg_f32_choose(len(n), *n3)
        own64 = lib.ins_dbg_spectral_choose(len(n), *n3, None, None) >= ROUTE_OWN2D
    assert got == route
    assert got != WRAP  # only ins_poisson_wrap_f32 makes that one
    if got in (FP64_SPECTRA, FLOAT2_SPECTRA):  # both run the fp64 solver's own passes
        assert own64 and len(n) == 3


def test_boxes_without_own_passes_are_what_the_table_says():
    """the rows that put a z side of the float2 kernel under sides without own passes rest on the fp64 chooser saying so"""
    from ins_amd import _lib

    lib = _lib.load()
    for n in ((24, 20, 256), (48, 16, 384), (128, 20, 192), (66, 16, 512)):
        assert lib.ins_dbg_spectral_choose(3, *n, None, None) < ROUTE_OWN2D, n
