"""The spectral Poisson solver's route (csrc/ins_poisson.hip: ins_spectral_choose) without a device: the choice for a box under the switches that
select it, written out from the conditions the solver had before the route was a value of its own; and the two symbol permutations (the storage order
in which a route's y pass leaves ky) against their inverse maps."""
import ctypes as C

import numpy as np
import pytest

# SpectralRoute / KyOrder of csrc/ins_internal.h
ROCFFT, ROCFFT_ZFUSED, OWN2D, OWN2D_ONE, OWN_LDS, OWN_LINE3, OWN_XY, OWN_YZ = range(8)
NATURAL, DIGITREV, LINE3 = range(3)
KY_OF = {ROCFFT: NATURAL, ROCFFT_ZFUSED: NATURAL, OWN2D: NATURAL, OWN2D_ONE: NATURAL, OWN_LDS: DIGITREV, OWN_XY: DIGITREV, OWN_YZ: DIGITREV,
         OWN_LINE3: LINE3}

POW2 = [16, 32, 64, 128, 256, 512, 1024]
MIXED = [96, 192, 384, 160, 320, 640]  # 3 * 2^m, 5 * 2^m


def choose(lib, n):
    ky, parts = C.c_int32(-1), C.c_int32(-1)
    route = lib.ins_dbg_spectral_choose(len(n), n[0], n[1], n[2] if len(n) == 3 else 1, C.byref(ky), C.byref(parts))
    return route, ky.value, parts.value


# (box, switches, route, partitions: exact count, or None for "the library's choice, at least 2")
TABLE = [
    ((256, 256, 256), {}, OWN_LINE3, 0),
    ((16, 128, 16), {}, OWN_LINE3, 0),
    ((16, 256, 32), {}, OWN_LINE3, 0),
    ((192, 384, 192), {}, OWN_LINE3, 0),
    ((64, 64, 64), {}, OWN_XY, 0),
    ((16, 16, 192), {}, OWN_XY, 0),
    ((128, 32, 16), {}, OWN_LDS, 0),
    ((24, 20, 16), {}, ROCFFT_ZFUSED, 0),
    ((12, 20, 8), {}, ROCFFT, 0),
    ((64, 64), {}, OWN2D_ONE, 0),
    ((1024, 32), {}, OWN2D, 0),
    ((4096, 4096), {}, ROCFFT, 0),
    ((256, 256, 256), dict(INS_DISABLE_LINE3=1), OWN_LDS, 0),
    ((64, 64, 64), dict(INS_DISABLE_XYFUSED=1), OWN_LDS, 0),
    ((64, 64, 64), dict(INS_DISABLE_OWNFFT=1), ROCFFT_ZFUSED, 0),
    ((192, 192, 192), dict(INS_OWNFFT_POW2_ONLY=1), ROCFFT, 0),
    # INS_YZ_FUSED alone leaves the partition count to ins_ownfft_yz_partitions, which wants 128 workgroups (tiles of 8 kx times partitions of at
    # least 8 planes): a box as narrow as (32, 128, 64) has 3 tiles x 8 partitions and stays on five passes; a forced count takes it
    ((32, 128, 64), dict(INS_YZ_FUSED=1), OWN_LINE3, 0),
    ((32, 128, 64), dict(INS_YZ_FUSED=1, INS_YZ_PARTITIONS=2), OWN_YZ, 2),
    ((32, 128, 64), dict(INS_YZ_PARTITIONS=8), OWN_YZ, 8),
    ((256, 128, 64), dict(INS_YZ_FUSED=1), OWN_YZ, None),
    ((128, 128, 256), dict(INS_YZ_FUSED=1), OWN_YZ, 16),
    ((32, 128, 64), dict(INS_YZ_FUSED=1, INS_DISABLE_YZ_FUSED=1), OWN_LINE3, 0),
    ((32, 128, 64), dict(INS_YZ_FUSED=1, INS_YZ_PARTITIONS=2, INS_DISABLE_YZ_FUSED=1), OWN_LINE3, 0),
    ((256, 128, 64), dict(INS_YZ_FUSED=1, INS_DISABLE_LINE3=1), OWN_YZ, None),  # the four-pass route rides on the LDS y passes
    ((24, 20, 16), dict(INS_DISABLE_ZSOLVE=1), ROCFFT, 0),
    ((64, 64), dict(INS_DISABLE_XYFUSED=1), OWN2D, 0),
    ((64, 64), dict(INS_DISABLE_OWNFFT=1), ROCFFT, 0),
]


@pytest.mark.parametrize("n,opts,route,parts", TABLE)
def test_route_chosen_for_a_box(n, opts, route, parts):
    from ins_amd import _lib

    lib = _lib.load()
    with _lib.options(**opts):
        got, ky, p = choose(lib, n)
    assert got == route
    assert ky == KY_OF[route]
    assert p >= 2 if parts is None else p == parts
    assert (p > 0) == (route == OWN_YZ)


def permuted(lib, order, n):
    """out[position] = frequency held there, from the library's symbol permutation applied to ay[k] = k"""
    ay, out = np.arange(n, dtype=np.float64), np.full(n, -1.0)
    lib.ins_dbg_permute_ky(order, n, ay.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert sorted(out) == list(range(n))  # a permutation
    return out.astype(int)


def digitrev_freq_of_pos(n, p):
    """Inverse of ins_ownfft_permute_symbol: the frequency at storage position p after the radix-3 / radix-5 stage (if any), the radix-2 stage
    (odd log2) and the radix-4 stages of the decimation-in-frequency passes — one digit of k per stage, least significant first."""
    r = 5 if n % 5 == 0 else (3 if n % 3 == 0 else 1)
    L = n // r
    k, mult = 0, 1
    radices = ([r] if r != 1 else []) + ([2] if (L.bit_length() - 1) % 2 else []) + [4] * ((L.bit_length() - 1) // 2)
    L = n
    for radix in radices:
        L //= radix
        q, p = divmod(p, L)
        k += q * mult
        mult *= radix
    return k


@pytest.mark.parametrize("n", POW2 + MIXED)
def test_digit_reversed_symbol_permutation_against_its_inverse(n):
    from ins_amd import _lib

    freq = permuted(_lib.load(), DIGITREV, n)
    assert [digitrev_freq_of_pos(n, p) for p in range(n)] == list(freq)


@pytest.mark.parametrize("n", [128, 256, 512] + MIXED)  # the lengths k_line3 has
def test_line3_symbol_permutation_against_its_inverse(n):
    from ins_amd import _lib

    lib = _lib.load()
    freq = permuted(lib, LINE3, n)
    assert [lib.ins_dbg_line3_pos_of_freq(n, int(k)) for k in freq] == list(range(n))


def test_natural_order_is_the_identity():
    from ins_amd import _lib

    assert list(permuted(_lib.load(), NATURAL, 20)) == list(range(20))
