"""The approximated harmonic centrality job restated for the tests, on top of tests/ampc_ref.py and tests/ampc_round_ref.py: what
hbu_fold_harmonic, hbu_graph_node_sketch and hbu_export of include/hb_ampc.h and run_approx_harmonic_job of stract_amd/ampc.py must compute.
Written from the reference's semantics: approximated_harmonic_centrality/coordinator.rs:82-148 (num_samples, norm, the loop over the sampled
sources, the fold of res.distances.iter()), kahan_sum.rs:44-72 (From<f64>, AddAssign<KahanSum>), hyperloglog.rs:4385-4400 and 4531-4535
(HyperLogLog<4096>::add / add_u128 / merge), shortest_path/worker.rs:44-49 (the worker's node sketch).  Floats are numpy.float64 inside (inf
and NaN instead of Python's exceptions), KahanSum = (sum, err) of Python floats, ids are Python ints (u128)."""
import math
import struct

import numpy as np

from tests import ampc_round_ref as rref

M64 = (1 << 64) - 1
LARGE_PRIME = rref.LARGE_PRIME
SKETCH_REGISTERS = 4096
SKETCH_B = 12


def bits(x):
    """the bit pattern of an f64; every NaN as one pattern (a NaN's sign and payload are not pinned: x86 and gfx950 differ on inf - inf)"""
    return 0x7FF8000000000000 if x != x else struct.unpack("<Q", struct.pack("<d", x))[0]


def kahan_bits(k):
    return (bits(k[0]), bits(k[1]))


def kahan_add_kahan(k, rhs):
    """KahanSum += KahanSum, kahan_sum.rs:65-72"""
    with np.errstate(all="ignore"):
        s, e = np.float64(k[0]), np.float64(k[1])
        y = (np.float64(rhs[0]) + np.float64(rhs[1])) - e
        t = s + y
        return (float(t), float((t - s) - y))


def harmonic_term(distance, norm):
    """(1.0 / distance as f64) * norm, coordinator.rs:140; `as f64` rounds to nearest even, as Python's float(int) does"""
    with np.errstate(all="ignore"):
        return float((np.float64(1.0) / np.float64(float(distance))) * np.float64(norm))


def fold(centralities, distances, norm, skip_zero=False):
    """coordinator.rs:139-145 for one finished job: entry().and_modify(|sum| *sum += centrality).or_insert(centrality).  Returns (folded,
    inserted).  skip_zero: the defined difference HBU_FOLD_SKIP_ZERO."""
    folded = inserted = 0
    for node, d in distances.items():
        if skip_zero and d == 0:
            continue
        c = (harmonic_term(d, norm), 0.0)  # KahanSum::from
        if node in centralities:
            centralities[node] = kahan_add_kahan(centralities[node], c)
        else:
            centralities[node] = c
            inserted += 1
        folded += 1
    return folded, inserted


def fold_fused(k, distance, norm):
    """what the fold must NOT compute: y = fma(1 / d, norm, -err), one rounding where the reference has two.  Exact rational arithmetic, then
    one rounding to nearest (finite values only)."""
    from fractions import Fraction
    q = float(np.float64(1.0) / np.float64(float(distance)))
    y = float(Fraction(q) * Fraction(norm) - Fraction(k[1]))  # float(Fraction) rounds to nearest even
    t = k[0] + y
    return (t, (t - k[0]) - y)


def num_samples(num_nodes, sample_rate):
    """coordinator.rs:82-84"""
    n = float(num_nodes)
    v = (math.log2(n) if n > 0 else -math.inf) / (sample_rate * sample_rate)
    return min(max(int(math.ceil(v)), 0), M64) if math.isfinite(v) else (M64 if v > 0 else 0)


# ---- HyperLogLog<4096> ----------------------------------------------------------------------------------------------------------------
def sketch_register(node):
    """(j, p) of add_u128(node): the high half of the id is dropped"""
    h = ((node & M64) * LARGE_PRIME) & M64
    w = (h << SKETCH_B) & M64
    return h >> (64 - SKETCH_B), (64 - w.bit_length()) + 1  # leading_zeros(0) = 64: p = 65


def sketch(nodes):
    reg = np.zeros(SKETCH_REGISTERS, dtype=np.uint8)
    for n in nodes:
        j, p = sketch_register(n)
        reg[j] = max(int(reg[j]), p)
    return reg


def sketch_merge(a, b):
    """merge(), hyperloglog.rs:4531-4535"""
    return np.maximum(a, b)


# ---- the coordinator --------------------------------------------------------------------------------------------------------------------
def run_job(rounds):
    """a generator of tests/ampc_round_ref.py to its return value"""
    while True:
        try:
            next(rounds)
        except StopIteration as done:
            return done.value


def approx_harmonic_job(workers, sampled_nodes, n_samples, max_distance, skip_zero=False):
    """coordinator.rs:107-148 over workers [(nodes, edges)]: yields (centralities, folded, inserted) after every source (the live dict
    node -> KahanSum); the generator's return value is {node: f64::from(sum)}."""
    with np.errstate(all="ignore"):
        norm = float(np.float64(1.0) / np.float64(float(n_samples - 1)))
    centralities = {}
    for source in sampled_nodes:
        distances = run_job(rref.shortest_path_job(workers, source, max_distance))
        folded, inserted = fold(centralities, distances, norm, skip_zero)
        yield centralities, folded, inserted
    return {n: k[0] for n, k in centralities.items()}


# The contraction case: one node folded six times with these distances at num_samples = 2658.  With y = fma(1 / d, norm, -err) the last
# fold leaves err = -2^-64 where the reference's two roundings leave -2^-65 (tests/test_ampc_approx_ref.py re-derives both).
CONTRACTION_NUM_SAMPLES = 2658
CONTRACTION_DISTANCES = (1, 6, 5, 6, 3, 2)
