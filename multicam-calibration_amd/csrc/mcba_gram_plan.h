// mcba_gram_plan.h -- which launches linearise one shard (k_gram and its variants, mcba_kernels.hip), as a value: the plan, the pure
// function that makes it from the shard's shape, and what the host derives from it -- grids, LDS, the point-chunk scratch, and where
// k_syrk's decision prologue finds the trial cost.  Host arithmetic without a HIP include: tests/hostcheck/gram_plan_hostcheck.cpp
// compiles it with g++, tests/test_hostcheck_gram_plan.py holds it to the rules it replaced (tests/gram_plan_oracle.py).
#pragma once
#include <stddef.h>

namespace mcba {

constexpr int kGramRaw = 88;  // ee 21 | he 6 | cost | ii 17 | ie 36 | hi 6 | any
constexpr int kGramRawA = 29, kGramRawB = 59;  // what role A / role B of the expansion needs of them
// doubles of the LDS exchange area of a point-split workgroup (gram_body MODE 3): npw wavefronts per group, with / without role B
constexpr int gram_xch_doubles(int npw, bool with_b) {
  return npw == 4 ? (with_b ? (4 * kGramRawA + 3 * 32 + 3 * 27) * 64 : 4 * kGramRawA * 64) : (4 / npw) * (npw - 1) * (with_b ? kGramRaw : kGramRawA) * 64;
}
constexpr size_t kGramPsplitLdsMax = (size_t)gram_xch_doubles(4, true) * sizeof(double);  // the largest exchange area: what the LDS opt-in of the point split asks for

// The launch variants, by the code MCBA_GRAM_SPLIT takes and GramPlan::split keeps:
//   0  fused: both accumulator sets in one lane, one wavefront per SIMD (k_gram)
//   1  split roles: two roles, two wavefronts per SIMD (k_gram_split) -- few frames
//   2  whole rounds of the wavefront slots fused + the short last round as split roles
//   3  whole rounds fused + the last round's POINTS in nchunk chunks over the idle SIMDs (k_gram_chunk, k_gram_combine)
//   4  point split inside the workgroup: npw wavefronts per (camera, frame block) meet in LDS (k_gram_psplit)
//   5  whole rounds fused + the last round point-split, in one launch (k_gram_mixed)
// A camera block 6 wide (the intrinsics held fixed) runs role A alone: the point split (4), else the role-A half of the split roles (1).
enum GramKind { GRAM_FUSED, GRAM_ROLES, GRAM_PSPLIT, GRAM_ROLE_A };
enum GramTail { GRAM_TAIL_NONE, GRAM_TAIL_ROLES, GRAM_TAIL_CHUNKS, GRAM_TAIL_PSPLIT };

// a shard as the planner sees it: C cameras x nfb blocks of 64 frames, N board points, `slots` wavefront slots of the device at one
// wavefront per SIMD (4 x compute units), camera block width cw, whether the device grants k_gram_psplit its LDS, and the two tuning
// knobs (MCBA_GRAM_SPLIT 0 .. 5, MCBA_GRAM_NPW 2 / 4; -1 = not set)
struct GramShape { int C, nfb, N, slots, cw; bool psplit_ok; int force_split, force_npw; };

// frame blocks (a multiple of 4: whole workgroups of the fused kernel) that whole rounds of the wavefront slots cover: the head.  The one
// place this cut is computed -- the chunk scratch and k_syrk's cost slots depend on it through the plan
inline int gram_round_blocks(int C, int nfb, int slots) { return ((C * nfb / slots) * slots / C) & ~3; }

struct GramCostSlots { int cstride, cinner, cdense; };  // see SyrkFuse (mcba_kernels.h)

struct GramPlan {
  int C = 0, nfb = 0;
  GramKind whole = GRAM_FUSED;      // what runs on the frame blocks [0, nfb) -- with a tail: GRAM_FUSED, on [0, head)
  GramTail tail = GRAM_TAIL_NONE;   // what runs on [head, nfb)
  bool with_b = true;               // false: role A alone (camera block 6 wide)
  int head = 0;                     // gram_round_blocks, whether a tail is launched or not
  int npw = 4;                      // point split: wavefronts per (camera, frame block), 4 or 2
  int nchunk = 0, ppc = 0, nrun = 0;  // point chunks: chunks the scratch holds per (camera, frame block), points per chunk, chunks that have points
  int split = 0;                    // the variant asked for (0 .. 5, above), before "no usable tail means fused": for messages and the profile scripts
  bool refused = false;             // MCBA_GRAM_SPLIT = 4 / 5 where the device cannot give the point split its LDS: nothing to launch

  int fused_blocks() const { return tail == GRAM_TAIL_NONE ? nfb : head; }
  int tail_blocks() const { return tail == GRAM_TAIL_NONE ? 0 : nfb - head; }
  // grid.x per camera: workgroups of four wavefronts with a frame block each; point-split workgroups of 4 / npw frame blocks
  static int quads(int blocks) { return (blocks + 3) / 4; }
  int psplit_groups(int blocks) const { return (blocks + 4 / npw - 1) / (4 / npw); }
  size_t psplit_lds_bytes() const { return (size_t)gram_xch_doubles(npw, with_b) * sizeof(double); }
  size_t chunk_doubles() const { return tail == GRAM_TAIL_CHUNKS ? (size_t)C * (nfb - head) * nchunk * kGramRaw * 64 : 0; }
  // k_gram leaves the cost of a workgroup (four frame blocks) in its first wavefront's slot, zeros in the others; the point split one
  // cost per frame block
  GramCostSlots cost_slots() const {
    if (whole == GRAM_PSPLIT) return {4, nfb, 0};
    if (tail == GRAM_TAIL_PSPLIT) return {4, head / 4 + nfb - head, head / 4};
    return {4, quads(nfb), 1 << 30};
  }
};

inline GramPlan gram_plan(const GramShape& s) {
  const int C = s.C, nfb = s.nfb, N = s.N, slots = s.slots, items = C * nfb;
  GramPlan p;
  p.C = C; p.nfb = nfb; p.with_b = s.cw != 6;
  p.head = gram_round_blocks(C, nfb, slots);
  const int tail = C * (nfb - p.head);
  // a short last round behind at least one whole one: what the three tail variants are for
  const bool short_tail = items > slots && p.head > 0 && tail > 0 && tail <= slots / 2;
  // point chunks pay for large boards only (the chunk + combine launches cost ~25 us whatever the board: break-even near 90 points),
  // at most 8 of them, no more than fill the idle slots, 8 points each at least -- and two chunks or it is no split
  int nchunk = 0;
  if (short_tail && N >= 128) nchunk = slots / tail < 8 ? slots / tail : 8;
  if (nchunk > N / 8) nchunk = N / 8;
  if (nchunk < 2) nchunk = 0;
  // ---- what the shape asks for
  const bool ps = s.psplit_ok;
  int split, npw = 4;
  if (ps && items <= slots / 4) split = 4;                         // at most a quarter of the slots: four wavefronts per item
  else if (ps && items <= slots / 2) { split = 4; npw = 2; }       // at most half: two
  else if (ps && items <= slots) split = 0;                        // (measured at 6 x 7 000 x 54, 660 items: fused 47.4 us, split roles 53.2 us)
  else if (ps && short_tail && tail <= slots / 4) split = 5;
  else if (nchunk) split = 3;                                      // (24 x 6250 x 200: k_gram 381 -> 360 us)
  else if (ps && short_tail) { split = 5; npw = 2; }
  else if (items > 2 * slots && items % slots > 0 && items % slots <= slots / 2) split = 2;   // (24 x 6250 x 200, 2.3 rounds: 536 us vs 561 us fused, 612 us split)
  else split = items < 3 * slots / 4 || (items > slots && items <= 3 * slots / 2);   // under-filled rounds: the split roles double the wavefronts
  // ---- the tuning knobs
  if (s.force_split >= 0) {
    split = s.force_split;
    if (split == 3 && !nchunk) nchunk = N / 8 < 2 ? 2 : N / 8 > 4 ? 4 : N / 8;
    if (split >= 4 && !ps) { p.refused = true; return p; }
  }
  if (s.force_npw >= 0) npw = s.force_npw == 2 ? 2 : 4;
  if (!p.with_b && split != 4) split = 1;
  // ---- what is launched: 2 / 3 / 5 without a usable tail are the fused kernel
  p.split = split;
  p.npw = npw;
  const bool cut = p.head > 0 && p.head < nfb;
  if (split == 4) p.whole = GRAM_PSPLIT;
  else if (split == 1) p.whole = p.with_b ? GRAM_ROLES : GRAM_ROLE_A;
  else if (split == 2 && cut) p.tail = GRAM_TAIL_ROLES;
  else if (split == 5 && cut) p.tail = GRAM_TAIL_PSPLIT;
  if (split == 3) p.nchunk = nchunk;
  if (split == 3 && cut) {
    p.tail = GRAM_TAIL_CHUNKS;
    p.ppc = ((N + nchunk - 1) / nchunk + 3) & ~3;   // (a multiple of the point loop's four)
    p.nrun = (N + p.ppc - 1) / p.ppc;
  }
  return p;
}

}  // namespace mcba
