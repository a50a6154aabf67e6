// hb_experiments.h - switches of the EXPERIMENTS build of the library (-DHB_EXPERIMENTS: `make exp` -> stract_amd/lib/libhyperball_exp.so,
// and the SIMT-interpreter test build).  NOT part of the product: the shipped libhyperball.so compiles none of this in and hb_create
// refuses an hb_options that sets any of these bits (include/hyperball.h documents only what an integrator may set).
//
// What lives here: A/B switches of measured-and-rejected kernel forms (kept so that their measurements stay reproducible and their
// parity tests keep running: DESIGN.md "tried and rejected"), and test hooks that force rarely taken paths at small sizes.
// stract_amd/_lib.py loads the experiments build by itself when a test asks for one of them.
//
//   hb_options.tune[1], bits above the low byte (the low byte - gather unroll - is a product knob): the HB_X_* names below, one per switch
//   hb_options.tune[7]  hottest counters staged in LDS by the level-1 dense launch (0 = off, <= 2048; measured slower, round 2)
#pragma once
#include <stdint.h>

#define HB_TUNE1_UNROLL 0xFFu // the low byte of tune[1]: the gather unroll, a product knob
#ifdef HB_EXPERIMENTS
#define HB_XBITS(tune1) ((uint32_t)(tune1) & ~HB_TUNE1_UNROLL)
#else
#define HB_XBITS(tune1) 0u
#endif

// The switches in hb_options.tune[1] (stract_amd/_lib.py carries the same names and values; tests/test_host.py compares the two)
enum hb_xbit : uint32_t {
    HB_X_TILE_EPILOGUE = 0x100u,          // bit  8  dense fused node rows with the per-tile estimator / Kahan epilogue instead of the once-per-row one (round 3 A/B)
    HB_X_SEED_3LAUNCH = 0x800u,           // bit 11  sweep passes always with the three-launch seed collection / expansion, also in the convergence tail
    HB_X_NO_EDGE_OVERLAP = 0x1000u,       // bit 12  edge partition without the merge / all-reduce / epilogue pipeline over row ranges
    HB_X_BITMAP_SLOTWISE = 0x2000u,       // bit 13  bitmap passes gather slot by slot instead of packing each row's surviving sources first (round 2 form)
    HB_X_NO_STAGED_RESULTS = 0x4000u,     // bit 14  staged result download off (hb_finish ships the whole image)
    HB_X_SNAPSHOT_EVERY_PASS = 0x8000u,   // bit 15  a result snapshot after EVERY pass, whatever the graph's size (tests: small graphs)
    HB_X_SHORT_FINAL_LIST = 0x10000u,     // bit 16  a final list of 16 entries (tests: the overflow path)
    HB_X_ONE_SNAPSHOT = 0x20000u,         // bit 17  one snapshot only
    HB_X_NO_TAIL_PIPELINE = 0x100000u,    // bit 20  hb_run's tail pipeline off
    HB_X_TAIL_KERNEL = 0x200000u,         // bit 21  the far tail as one workgroup (hb_tail.hip.h) after a small sweep pass; measured no faster (round 5)
    HB_X_TAIL_KERNEL_ANY = 0x400000u,     // bit 22  ... after any pass (tests)
    HB_X_FULL_INIT = 0x800000u,           // bit 23  hb_begin always writes the whole initial state (round 6 A/B: the lean pass 0 off)
    HB_X_WIRE_64B = 0x1000000u,           // bit 24  destination partition, changed-only: 64-byte counters on the wire instead of the 6-bit packing (round 6 A/B)
    HB_X_SCATTER_TRANSPOSE = 0x2000000u,  // bit 25  the transposed work-row graph by atomic scatter (the form before round 6; today only the out-of-memory fallback)
    HB_X_SWEEP_ROUNDS = 0x4000000u,       // bit 26  sweep passes: a touched row's sources 8 per round (index / bit word / gather each a round trip) instead of all at once
    HB_X_GENERIC_LEVEL1 = 0x8000000u,     // bit 27  pass 0: the first hub-chunk level through the generic INIT kernel instead of init_level1_kernel (A/B)
    HB_X_PROBE_NO_SIZE = 0x10000000u,     // bit 28  TIMING PROBE, WRONG RESULTS: the dense fused node rows neither read nor write size[] (16 B per row less state traffic)
    HB_X_SIM_SMALL_PIECES = 0x20000000u,  // bit 29  hb_inbound_similarity with a limit: the cut lists are built in pieces of 64 hosts instead of 65536 (tests: several pieces)
};
