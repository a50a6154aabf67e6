"""tests/ampc_approx_ref.py against what the reference states about itself and against answers derived by hand: the model the GPU tests
of tests/test_ampc_approx.py compare with must itself be right.  No GPU."""
import math

from stract_amd import ampc
from tests import ampc_approx_ref as aref
from tests import ampc_ref as ref

INF, NAN_BITS = math.inf, 0x7FF8000000000000


def test_kahan_sum_known_answer_of_the_reference():
    """kahan_sum.rs `it_works_kahan`: 10000, pi, e, pi, e, pi, e added as KahanSum::from(elem) give 10017.579623446147 - and so does `+= f64`
    (`it_works`), which is the operator the composed route's KAHAN_ADD uses"""
    a, b = ref.KAHAN_DEFAULT, ref.KAHAN_DEFAULT
    for x in [10000.0, math.pi, math.e, math.pi, math.e, math.pi, math.e]:
        a = aref.kahan_add_kahan(a, (x, 0.0))
        b = ref.kahan_add(b, x)
    assert a[0] == 10017.579623446147 and aref.kahan_bits(a) == aref.kahan_bits(b)
    # rhs.err counts: (1.0, 2^-60) is not (1.0, 0.0)
    assert aref.kahan_add_kahan((0.0, 0.0), (1.0, 2.0 ** -52)) == (1.0 + 2.0 ** -52, 0.0)


def test_num_samples():
    """coordinator.rs:82-84; the issue's figure for 10^8 nodes at rate 0.1"""
    want = {(10 ** 8, 0.1): 2658, (1, 0.1): 0, (2, 1.0): 1, (1000, 0.5): 40, (0, 0.1): 0, (1 << 40, 0.05): 16000, (3, 0.3): 18}
    for (n, rate), v in want.items():
        assert aref.num_samples(n, rate) == v, (n, rate)
        assert ampc.num_samples(n, rate) == v, (n, rate)


def test_harmonic_term_conversions():
    """`distance as f64` rounds to nearest even: 2^53 + 1 is 2^53, 2^64 - 1 is 2^64; distance 0 is inf"""
    assert aref.harmonic_term((1 << 53) + 1, 1.0) == 2.0 ** -53
    assert aref.harmonic_term((1 << 64) - 1, 1.0) == 2.0 ** -64
    assert aref.harmonic_term(0, 0.5) == INF and aref.harmonic_term(3, INF) == INF
    assert aref.harmonic_term(3, 1.0 / 3.0) == (1.0 / 3.0) * (1.0 / 3.0)


def test_path_graph_by_hand():
    """a -> b -> c, sources [a, b], num_samples = 3: norm = 1/2.  From a: a 0, b 1, c 2 -> inf, 1/2, 1/4.  From b: b 0, c 1 -> inf, 1/2.
    b holds 1/2 when inf arrives: t = inf, err = (inf - 1/2) - inf = NaN.  c = 1/4 + 1/2 exactly."""
    a, b, c = 10, 20 | (1 << 64), 30
    workers = [([a, b], [(a, b)]), ([c], [(b, c)])]
    job = aref.approx_harmonic_job(workers, [a, b], 3, 5)
    cent, folded, inserted = next(job)
    assert (folded, inserted) == (3, 3) and cent == {a: (INF, 0.0), b: (0.5, 0.0), c: (0.25, 0.0)}
    cent, folded, inserted = next(job)
    assert (folded, inserted) == (2, 0)
    assert {n: aref.kahan_bits(k) for n, k in cent.items()} == {a: aref.kahan_bits((INF, 0.0)), b: (aref.bits(INF), NAN_BITS), c: aref.kahan_bits((0.75, 0.0))}
    assert aref.run_job(job) == {a: INF, b: INF, c: 0.75}
    # the defined difference: the sources' own zero distances stay out (a is reached by nobody: absent)
    assert aref.run_job(aref.approx_harmonic_job(workers, [a, b], 3, 5, skip_zero=True)) == {b: 0.5, c: 0.75}
    # max_distance = 1: one round per source, c is reached from b only
    assert aref.run_job(aref.approx_harmonic_job(workers, [a, b], 3, 1, skip_zero=True)) == {b: 0.5, c: 0.5}


def test_zero_distance_three_times():
    """inf, then err = NaN, then sum = NaN"""
    cent = {}
    seen = []
    for _ in range(3):
        aref.fold(cent, {7: 0}, 0.5)
        seen.append(aref.kahan_bits(cent[7]))
    assert seen == [(aref.bits(INF), 0), (aref.bits(INF), NAN_BITS), (NAN_BITS, NAN_BITS)]


def test_contraction_case_differs_when_fused():
    """The fixture the GPU test folds: with y = fma(1 / d, norm, -err) the sixth fold ends with err = -2^-64, as written (two roundings)
    with -2^-65; the sums agree.  A fold compiled with floating-point contraction fails tests/test_ampc_approx.py on it."""
    norm = 1.0 / (aref.CONTRACTION_NUM_SAMPLES - 1)
    assert aref.CONTRACTION_NUM_SAMPLES == aref.num_samples(10 ** 8, 0.1)
    written = fused = None
    for d in aref.CONTRACTION_DISTANCES:
        v = aref.harmonic_term(d, norm)
        written = (v, 0.0) if written is None else aref.kahan_add_kahan(written, (v, 0.0))
        fused = (v, 0.0) if fused is None else aref.fold_fused(fused, d, norm)
    assert written[1] == -(2.0 ** -65) and fused[1] == -(2.0 ** -64)
    assert aref.kahan_bits(written) != aref.kahan_bits(fused)
    assert written[0] == fused[0] == 0.0008907288922343495


def test_sketch_registers():
    """HyperLogLog<4096>::add by hand: id 0 hashes to 0 (register 0, p = 65); the inverse of the prime hashes to 1 (register 0, p = 52);
    the high half of an id is dropped; merge is the byte-wise max"""
    inv = pow(aref.LARGE_PRIME, -1, 1 << 64)
    assert aref.sketch_register(0) == (0, 65)
    assert aref.sketch_register(inv) == (0, 52)  # h = 1: h << 12 has 51 leading zeros
    assert aref.sketch_register((inv * ((4095 << 52) | (1 << 51))) & aref.M64) == (4095, 1)
    assert aref.sketch_register(12345 | (9 << 64)) == aref.sketch_register(12345)
    assert not aref.sketch([]).any()
    a, b = aref.sketch([inv, 5, 6]), aref.sketch([0, 7])
    assert a[0] == 52 and b[0] == 65
    assert (aref.sketch_merge(a, b) == aref.sketch([inv, 5, 6, 0, 7])).all()
