// gemm_x6p.hip - K2p: the split-f32 (x6) encoder GEMM with its weights split once, at
// load time, into the fragment-blocked W3 image (gemm_x6p.hpp), replacing the x6 tiles of
// gemm_f32.hpp that re-split BOTH operands on every K-slice in every workgroup.
//
// out[M,N] = epi(A[M,K] . W[N,K]^T + bias (+ resid)), A fp32, W as W3 (3 bf16 planes).
//
//  * one 512-thread workgroup per CU (8 waves, two per SIMD), persistent over tiles;
//    block tile BM x BN = (WAVES_M 32 TM) x (WAVES_N 32 TN); a wave owns a 32 TM x 32 TN
//    tile as 2 TM x 2 TN accumulator blocks of v_mfma_f32_16x16x32_bf16 (X6pTile::M16,
//    every tile code below 16);
//  * K advances in 32-deep stages - two 16-deep sub-stages - through an NBUF-slot LDS ring
//    filled by LDS-DMA (global_load_lds_dwordx4, no VGPR round trip, no staging VALU), a
//    counted vmcnt and one s_barrier per stage; on the default tiles 4 loader waves issue
//    the DMAs beside 4 compute waves;
//  * W3 sub-stage: BN / 32 x 3 fragments of 1 KB, each one DMA wave-instruction.  Lane
//    (c = lane & 15, kq = lane >> 4) of a 16x16x32 operand holds k = 8 kq + j of row c: for
//    the 16-row half s of a fragment it reads the 16 B at (kq & 1) 512 + (16 s + c) 16 of
//    sub-stage kq >> 1 (each group of lanes the LDS serves together covers 16 distinct
//    16-B slots: conflict-free);
//  * A sub-stage: BM rows x 16 fp32 (64 B per row), 16 rows per DMA wave-instruction; the
//    four 16-B chunks of row R sit at slot chunk ^ g((R >> 2) & 3), g = {0, 1, 3, 2} (the
//    XOR goes on the DMA SOURCE address: the DMA destination is lane-linear).  The lane
//    reads chunks 2 (kq & 1), + 1 of row c of sub-stage kq >> 1.  ds_read_b128 is served in
//    the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; with g
//    every group reads 16 distinct 16-B slots, for this read and for the 32x32x16 one
//    (with the plain (R >> 2) & 3 the 16x16x32 read was 2-way: lanes 0-3 against 24-27);
//  * A fragments are split into their three bf16 planes in registers (split3: round to
//    nearest per plane, residuals exact), in sub-pieces of at most 2 VALU in the MFMA
//    gaps, and each 16x16 block takes the six products a2b0, a1b1, a0b2, a1b0, a0b1, a0b0
//    per 32-deep step: the operands and order of gemm_f32.hpp's M16 tiles, so the results
//    are bit-identical to those tiles;
//  * operands are single-buffered and reloaded in place (the M16 branch of
//    gemm_x6p_kernel has the slot plan);
//  * tile codes 16 / 17 keep the former k-step (v_mfma_f32_32x32x16_bf16 on 32x32 blocks,
//    16-deep stages, 4 ring slots, fragments double-buffered) to re-measure the two MFMA
//    shapes in one library; the chip holds a higher clock on 16x16x32 (1.13-1.16x at the
//    encoder's shapes);
//  * tiles are walked in GM-row bands (GM row tiles x all column tiles, column-major
//    inside a band), each XCD taking consecutive tiles: at M = 8192 an XCD's 32 CUs share
//    4 A row panels and 8 W3 column panels in its L2.
#include <algorithm>

#include "gemm_epi.hpp"
#include "gemm_x6p.hpp"

namespace mq {
namespace {

typedef __attribute__((address_space(3))) void x6p_lds_t;

// One LDS-DMA wave-instruction: 16 B from base + voff (per lane) to LDS[lds_dst + 16 lane].
// Inline asm (as thresh.hip's ring): a compiler-visible LDS-DMA is tracked as a pending
// LDS write and every later ds_read of the array would wait vmcnt(0), draining the ring.
__device__ __forceinline__ void x6p_glds(const void* base, unsigned voff, unsigned lds_dst) {
  // the base is workgroup-uniform; say so (the uniformity analysis loses it through some
  // of the tile walks' index arithmetic, and the asm needs an SGPR pair)
  const uint64_t b64 = (uint64_t)(uintptr_t)base;
  base = (const void*)(uintptr_t)(((uint64_t)__builtin_amdgcn_readfirstlane((unsigned)(b64 >> 32)) << 32) |
                                  (unsigned)__builtin_amdgcn_readfirstlane((unsigned)b64));
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(base), "s"(__builtin_amdgcn_readfirstlane(lds_dst))
               : "memory");
}

// g of the A stage's chunk swizzle (file header): {0, 1, 3, 2}
__device__ __forceinline__ int a_swz(int q) { return q ^ (q >> 1); }

// Exact 3-way bf16 split of 4 floats (gemm_f32.hpp's split3, same arithmetic) with the
// packing conversion as a compiler-visible fptrunc (v_cvt_pk_bf16_f32, round to nearest
// even) instead of inline asm, so that sched_group_barrier counts it as VALU.
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned cvt_pk_bf16(float lo, float hi) {
  float2_t v;
  v.x = lo;
  v.y = hi;
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_t));
}
__device__ __forceinline__ void split3v(floatx4 x, uint2 (&pl)[3]) {
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    const unsigned a = cvt_pk_bf16(x.x, x.y), b = cvt_pk_bf16(x.z, x.w);
    pl[p] = make_uint2(a, b);
    if (p < 2) {  // residual is exact in fp32
      x.x -= bf16_lo(a);
      x.y -= bf16_hi(a);
      x.z -= bf16_lo(b);
      x.w -= bf16_hi(b);
    }
  }
}

// MQ_X6P_DBG (measurement builds only; wrong results): tile codes 8-15 of
// mq_debug_gemm_x6p run tiles 1 / 0 with parts of the stage removed - 1 no DMA, 2 no
// split, 8 no fragment reads, 16 no A DMA, 32 no W3 DMA, 64 prologue DMAs only, 128 no
// barrier, 256 no W3 fragment reads, 512 no A fragment reads - to price each part (the epilogue cannot be dropped: the
// MFMAs would be dead code).
#if defined(MQ_X6P_DBG) && !defined(MQ_MEASUREMENT_BUILD)
#error "MQ_X6P_DBG computes wrong results: only a measurement build (-DMQ_MEASUREMENT_BUILD) may set it"
#endif

template <int WAVES_M_, int WAVES_N_, int TM_, int TN_, int NBUF_, int KS_ = 1, int DMAW_ = 8, bool SCHED_ = false,
          int DBG_ = 0, int DSTEP_ = 1, int BR0_ = 0, int PS_ = 4, bool LDR_ = false, bool M16_ = false,
          bool DEEP_ = false>
struct X6pTile {
  static constexpr int WAVES_M = WAVES_M_, WAVES_N = WAVES_N_, TM = TM_, TN = TN_, NBUF = NBUF_;
  static constexpr int KS = KS_;    // 16-deep k-steps per LDS stage (one barrier per stage)
  // DMAW: waves that issue the stage's DMAs (8: all; 4: waves 0-3, so that on every SIMD
  // one of its two waves never stops its MFMA stream to issue DMAs).  SCHED: the k-step
  // is laid out slot by slot (one MFMA per slot, sched_barrier between slots) with the
  // next k-step's fragment reads, this wave's DMAs and the next A fragment's split spread
  // over the slots, so that the split VALU issues in the MFMA shadow (left alone the
  // compiler sinks the split to the next k-step, in front of its MFMAs).
  static constexpr int DMAW = DMAW_;
  static constexpr bool SCHED = SCHED_;
  // SCHED slot plan: DMA t of the stage behind the MFMA of slot t * DSTEP (k-step 0), the
  // next B fragment reads two per slot from slot BR0 (skipping DMA slots), the split
  // pieces from slot PS on
  static constexpr int DSTEP = DSTEP_, BR0 = BR0_, PS = PS_;
  static constexpr int DBG = DBG_;  // measurement builds only (MQ_X6P_DBG)
  // LDR: WAVES_M x WAVES_N = 4 compute waves (one per SIMD) plus 4 loader waves that only
  // issue the stage DMAs (an LDS-DMA holds the issuing wave for ~60-185 cycles; a loader
  // wave pays that beside its SIMD's compute wave, whose MFMA stream it never interrupts)
  static constexpr bool LDR = LDR_;
  // M16 (the product tiles): the k-step on v_mfma_f32_16x16x32_bf16 - the wave's
  // TM x TN 32x32 blocks as 2 TM x 2 TN 16x16 blocks, one 32-deep step per stage (KS = 2),
  // same LDS image, same LDS read bytes and split VALU per unit of K (the M16 branch of
  // gemm_x6p_kernel).
  // DEEP: the ring runs NBUF stages ahead (every read of a stage is in the iteration
  // before the one that multiplies it; the barrier then waits for those reads).
  static constexpr bool M16 = M16_, DEEP = DEEP_;
  static constexpr int NW = WAVES_M * WAVES_N, THREADS = (LDR ? 2 * NW : NW) * 64;
  static constexpr int WM = TM * 32, WN = TN * 32, BM = WAVES_M * WM, BN = WAVES_N * WN;
  static constexpr int A_SUB = BM * 64;  // one k-step of A: 16 fp32 per row
  static constexpr int B_SUB = BN * 96;  // one k-step of W3: 16 k x 3 planes x 2 B per row
  static constexpr int STAGE = KS * (A_SUB + B_SUB);
  static constexpr int NA = BM / 16, NB = BN / 32 * 3;  // DMA wave-instructions per k-step
  static constexpr int NI = KS * (NA + NB);                    // ... per stage
  static constexpr int CNT_LO = NI / DMAW, REM = NI % DMAW, CNT_HI = CNT_LO + (REM ? 1 : 0);
  static_assert(DMAW == 8 || DMAW == 4, "DMA waves");
  static_assert(!LDR || DMAW == 4, "loader mode: the 4 loader waves issue every DMA");
  // stage issue distance: a stage's slot is free once its last k-step's fragments are in
  // registers - at KS = 1 that happens one iteration early (the fragments run one k-step
  // ahead), so the ring can run one stage further ahead
  static constexpr int AHEAD = KS == 1 || (M16 && DEEP) ? NBUF : NBUF - 1;
  static_assert(!M16 || (KS == 2 && SCHED), "16x16x32 body: slot-scheduled 32-deep stages");
  static_assert(!DEEP || M16, "DEEP is a 16x16x32 option");
#ifndef MQ_X6P_GM  // tuning default: 8 row tiles per band (half the W3 column blocks per XCD
#define MQ_X6P_GM 4  // round) measured the same at every headline shape (tools/gpu_ab_x6p.sh)
#endif
  static constexpr int GM = MQ_X6P_GM;  // row tiles per band of the tile walk
  static_assert(LDR ? NW == 4 : NW == 8, "8-wave workgroups");
  static_assert(!SCHED || (CNT_HI - 1) * DSTEP < TM * TN * 6 * (M16 ? 4 : 1), "DMAs per k-step slots");
  static_assert(AHEAD >= 2 && NBUF * STAGE <= 160 * 1024, "LDS ring");
};

// The split epilogue's kinds and the block rows (of a wave tile's 4) a compute wave hands to its
// SIMD partner (1 or 2; tools/gemm_x6p_bench.py --ab measures a library built with the other).
// MQ_X6P_SPLIT_BIAS builds the split form of the two bias kinds as well (measured, not shipped:
// DESIGN.md section 4).
#ifndef MQ_X6P_HS
#define MQ_X6P_HS 2
#endif
#ifndef MQ_X6P_SPLIT_BIAS
#define MQ_X6P_SPLIT_BIAS 0
#endif
constexpr bool epi_is_split(int epi) {
  return epi == EPI_GELU_ERF || epi == EPI_GELU_TANH || epi == EPI_GELU_ERF_LNFOLD || epi == EPI_GELU_TANH_LNFOLD ||
         (MQ_X6P_SPLIT_BIAS != 0 && (epi == EPI_BIAS || epi == EPI_BIAS_LNFOLD));
}

// FORMER (tile codes 20 / 21 of mq_debug_gemm_x6p and mq_debug_gemm_x6p_ln): the epilogues as
// they were before the loader waves took part - the producer's own global loads on every tile
// (no hand-off), the consumers' whole wave tile finished by its compute wave (no split) - kept to
// re-measure the two in one library.  Same results, bit for bit.
//
// The producer's hand-off (HAND: EPI_RESID_LN_STATS on the loader-wave tiles X6p0 / X6p1).  On
// the workgroup's LAST tile the loader wave prepares its SIMD partner's residual during the
// final k-stages: it loads the partner's 64 x 96 wave tile of the residual and its rows'
// partials (ln_tile_load), forms t = (r - mu) rho and writes it to LDS in accumulator order
// (ln_tile_write); after one more barrier the compute wave finishes its rows from LDS
// (store_wave_tile16_ln_stats<.., HAND>), with no residual or stats_in round trips of its own.
// Tiles before the last keep the global-load epilogue: the ring is carrying the next tile's
// prefetch then, and no slot is free.
//   Slot plan (S stages, stage k in slot k % 3, ring two stages ahead).  The loader's DMAs of
//   "stages" S and S + 1 (re-reads of the last stage, never multiplied) are not issued.  After
//   barrier B(S) (below) slot S % 3 holds stage S - 3, multiplied two iterations ago (S = 1: the
//   prologue's re-read of stage 0, landed; S = 2: nothing), and slot (S + 1) % 3 holds stage
//   S - 2, whose multiplies every compute wave finished before it arrived at B(S).  Slot
//   (S - 1) % 3 holds the last stage and is not touched.  t (4 waves x 24 KB) goes to those
//   two slots, waves 0 - 1 to the first, 2 - 3 to the second (2 x 24 KB <= STAGE).  The compute
//   waves' never-multiplied reads of "stage S" in the last iteration come from slot S % 3 and
//   return whatever is there: those registers are dead.
//   Barriers, per role (every wave of the workgroup executes each exactly once):
//                         compute waves                      loader waves
//     prologue  B(0)      before reading stage 0             after vmcnt: stage 0 landed
//     stage j   B(j + 1)  top of iteration j, j < S          stage j + 1 landed, j < S
//     hand-off  B(S + 1)  after iteration S - 1's MFMAs      after t is written, lgkmcnt(0)
//   i.e. S + 2 on both sides.  The loader issues the residual loads after B(S - 1) (S = 1:
//   after B(0)), when none of its DMAs is left to issue: the vmcnt(0) in front of B(S) covers
//   them, and at most 13 DMAs + 24 + 4 loads are outstanding.  It writes t between B(S) and
//   B(S + 1), beside the last stage's MFMAs.
template <class T, int EPI, bool FORMER = false>
__global__ __launch_bounds__(T::THREADS, 1) void gemm_x6p_kernel(const float* __restrict__ A, int lda,
                                                             const unsigned char* __restrict__ W3,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ resid, int ldr,
                                                             float* __restrict__ out, int ldo, int M, int N,
                                                             int K, int rx, LnFold lf, AttnEpi at) {
  __shared__ __attribute__((aligned(1024))) unsigned char lds[T::NBUF * T::STAGE];
  const unsigned lds0 = (unsigned)(uintptr_t)(x6p_lds_t*)lds;
  constexpr bool HAND = EPI == EPI_RESID_LN_STATS && T::LDR && T::M16 && !T::DEEP && T::NBUF == 3 && !FORMER;
  // ATTN (EPI_ATTN_BIAS / EPI_ATTN_LNFOLD, X6p0 only): the tile's W3 column blocks are gathered
  // per head - tile column index = head, blocks [Q d0-31 | K d0-31 | V d0-31 | Q d32-63 | K d32-63
  // | V d32-63], so compute wave wn holds Q | K | V of head dims 32 wn .. + 31 for two whole
  // 32-row sequences - and the epilogue is the attention itself (gemm_epi.hpp attn_wave_tile),
  // worked in the ring slot that is free at every tile end:
  //   stage j, a tile's last, sits in slot j % 3.  The compute waves read it in iteration j - 1
  //   and wait lgkmcnt(0) before B(j + 1), so past B(j + 1) no wave has a read of it in flight.
  //   The loader refills slot j % 3 (stage j + 3) only after B(j + 2), which the compute waves
  //   reach after their epilogue.  The four waves' staging (4 x kAttnStage <= STAGE) lives there.
  //   Slot (j + 1) % 3 holds stage j + 1 until B(j + 3): after the epilogue the compute waves
  //   read and split its operands again, as the prologue does, so the copies prefetched in
  //   iteration j are dead across the epilogue.
  //   Barriers, per role (every wave of the workgroup executes each exactly once):
  //                         compute waves                        loader waves
  //     prologue  B(0)      before reading stage 0               after vmcnt: stage 0 landed
  //     stage j   B(j + 1)  top of iteration j (tile's last      stage j + 1 landed
  //                         stage: after lgkmcnt(0))
  //     tile end  X(j)      in the epilogue, partials written    after issuing stage j + 2,
  //               (j % nst == nst - 1)        and lgkmcnt(0)     waiting on nothing
  //   i.e. S + 1 + n_tiles on both sides, ragged tiles included: nothing about a barrier
  //   depends on M.
  constexpr bool ATTN = epi_is_attn(EPI);
  static_assert(!ATTN || (T::LDR && T::M16 && !T::DEEP && T::NBUF == 3 && T::WAVES_M == 2 && T::WAVES_N == 2 &&
                          T::TM == 2 && T::TN == 3 && 4 * kAttnStage <= T::STAGE),
                "attention epilogue: the 128 x 192 loader-wave tile");
  static_assert(!HAND || (T::NW == 4 && 2 * T::WM * T::WN * 4 <= T::STAGE && T::WN == kLnPartW && T::STAGE % 1024 == 0),
                "hand-off: two wave tiles of t per ring slot");
  // SPLIT (the GELU consumer kinds on the loader-wave tiles X6p0 / X6p1): at a tile end the
  // compute wave hands the last HS of its MB = 4 block rows to its SIMD partner, the loader wave
  // of the same cw, and both finish their rows with the same store_wave_tile16 at the same time:
  // two VALU streams per SIMD instead of one (a single wave issues a VALU instruction every 4
  // cycles at best, the SIMD one every 2).  Nothing overlaps the next tile's k-loop: the two meet
  // again at the stage barrier they already share.
  //   Slot plan.  Stage j, a tile's last, sits in slot j % 3.  As for ATTN above, the compute
  //   waves wait lgkmcnt(0) before B(j + 1), so slot j % 3 is free from B(j + 1) to B(j + 2): the
  //   loader refills it (stage j + 3) only after B(j + 2), which every wave reaches after its
  //   part of the epilogue.  Compute wave cw writes its HS x NB16 handed accumulator blocks, 1 KB
  //   each (one ds_write_b128 per block, lane l at byte 16 l), to slot j % 3 at cw HS NB16 1 KB
  //   (4 HS 6 KB <= STAGE); the loader wave reads them back lane-identically: the same register
  //   image, the same function, the same bits.  Slots (j + 1) % 3 and (j + 2) % 3 - stage j + 1,
  //   whose operands the compute wave keeps in registers across the epilogue, and stage j + 2,
  //   being filled - are untouched.
  //   Barriers, per role (every wave of the workgroup executes each exactly once):
  //                         compute waves                        loader waves
  //     prologue  B(0)      before reading stage 0               after vmcnt: stage 0 landed
  //     stage j   B(j + 1)  top of iteration j (tile's last      stage j + 1 landed
  //                         stage: after lgkmcnt(0))
  //     tile end  X(j)      after iteration j's MFMAs, handed    after issuing stage j + 2 and the
  //               (j % nst == nst - 1)  rows written, lgkmcnt(0) loads of bias / s / row statistics
  //   i.e. S + 1 + n_tiles on both sides; no barrier depends on M, on N or on the path (whole or
  //   ragged) a wave tile takes.  The loader wave's stores are covered by the vmcnt(0) of its
  //   next wait_stages (or the one after its loop).
  constexpr int HS = MQ_X6P_HS;
  constexpr bool SPLIT = epi_is_split(EPI) && !FORMER && T::LDR && T::M16 && !T::DEEP && T::NBUF == 3 && T::TM == 2 &&
                         T::TN == 3;
  static_assert(!SPLIT || ((HS == 1 || HS == 2) && 4 * HS * 2 * T::TN * 1024 <= T::STAGE),
                "split epilogue: the handed blocks of the four compute waves fit one ring slot");
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int cw = T::LDR ? wave % T::NW : wave;  // compute wave index
  const int wm = cw / T::WAVES_N, wn = cw % T::WAVES_N;
  const int tiles_m = (M + T::BM - 1) / T::BM, tiles_n = (N + T::BN - 1) / T::BN;
  const int total = tiles_m * tiles_n;
  const int G = gridDim.x, per_xcd = G >> 3;
  const int xslot = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  // rx > 0: the tile grid is cut into 8 regions, rx column blocks x 8 / rx row blocks, and
  // the workgroups that share blockIdx.x % 8 (an XCD under round-robin dispatch; a speed
  // assumption, never a correctness one) walk one region - its W3 column panels stay in
  // that XCD's L2 for the whole launch instead of being re-read every round
  int m_lo = 0, rm = tiles_m, n_lo = 0, rn = tiles_n, loc = xslot, wstep = G, rtiles = total;
  if (rx > 0) {
    const Region rg = region_of(rx, blockIdx.x & 7, tiles_m, tiles_n);
    m_lo = rg.m_lo;
    rm = rg.rm;
    n_lo = rg.n_lo;
    rn = rg.rn;
    loc = blockIdx.x >> 3;
    wstep = per_xcd;
    rtiles = rm * rn;
  }
  const int n_tiles = loc < rtiles ? (rtiles - loc + wstep - 1) / wstep : 0;
  if (n_tiles == 0) return;
  const int nk = K >> 4;                 // 16-deep k-steps per tile
  const int nst = nk / T::KS;            // stages per tile (the launcher checks K % (16 KS) == 0)
  const int S = n_tiles * nst;           // stages of this workgroup
  const int nbw = (N + 31) >> 5;
  const int band_tiles = T::GM * rn;
  auto coords = [&](int i, int& m0, int& n0) {  // bands of GM row tiles, column-major inside
    const int t = i * wstep + loc;
    const int band = t / band_tiles;
    const int gm = min(T::GM, rm - band * T::GM);
    const int w = t - band * band_tiles;
    const int tc = w / gm;
    m0 = (m_lo + band * T::GM + (w - tc * gm)) * T::BM;
    n0 = (n_lo + tc) * T::BN;
  };

  // ---- DMA issue of stage `is_j` into a ring slot (past the last stage: the last again,
  // never multiplied).  Instruction `ins` of a stage: k-step ins / (NA + NB), then A rows
  // 16 ins' .. + 15 (ins' < NA) or W3 fragment ins' - NA = 3 (column block) + plane.
  int is_j = 0, is_i = 0, is_kt = 0, is_m0, is_n0;
  coords(0, is_m0, is_n0);
  // A chunk this lane moves: row 16 ins + (lane >> 2), slot lane & 3 -> chunk slot ^ g((row >> 2) & 3)
  const unsigned a_chunk = (unsigned)(((lane & 3) ^ a_swz((lane >> 4) & 3)) * 16);
  // DMA t (< CNT_HI) of this wave for the stage at is_j into slot `buf`
  auto issue_one = [&](int buf, int t) __attribute__((always_inline)) {
    if constexpr (T::DBG & 1) return;
    if constexpr (T::DBG & 64) {  // prologue DMAs only: the loop multiplies stale stages
      if (is_j >= T::AHEAD) return;
    }
    const int dw = T::LDR ? wave - T::NW : wave;  // DMA wave index
    if (dw < 0 || dw >= T::DMAW || (T::REM && t == T::CNT_HI - 1 && dw >= T::REM)) return;
    const unsigned dst = lds0 + (unsigned)(buf * T::STAGE);
    const int ins = dw + t * T::DMAW;
    const int ks = ins / (T::NA + T::NB), in = ins - ks * (T::NA + T::NB);
    const int kt = is_kt + ks;
    if (in < T::NA) {
      if constexpr (T::DBG & 16) return;
      const float* abase = A + (int64_t)is_m0 * lda + kt * 16;
      const unsigned voff = (unsigned)min(16 * in + (lane >> 2), M - 1 - is_m0) * (unsigned)lda * 4u + a_chunk;
      x6p_glds(abase, voff, dst + ks * T::A_SUB + in * 1024);
    } else {
      if constexpr (T::DBG & 32) return;
      const int b = in - T::NA, nbl = b / 3, p = b - nbl * 3;
      int nbg = min((is_n0 >> 5) + nbl, nbw - 1);
      if constexpr (ATTN) nbg = (nbl % 3) * (N / 96) + 2 * (is_n0 / T::BN) + nbl / 3;  // (H / 32 blocks per third)
      const unsigned char* wbase = W3 + ((size_t)(nbg * nk + kt) * 3 + p) * 1024;
      x6p_glds(wbase, (unsigned)lane * 16u, dst + T::KS * T::A_SUB + ks * T::B_SUB + b * 1024);
    }
  };
  auto advance = [&]() __attribute__((always_inline)) {
    if (is_j + 1 < S) {
      ++is_j;
      is_kt += T::KS;
      if (is_kt == nk) {
        is_kt = 0;
        ++is_i;
        coords(is_i, is_m0, is_n0);
      }
    }
  };
  auto issue = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < T::CNT_HI; ++t) issue_one(buf, t);
    advance();
  };

  // ---- fragments of one k-step (A split into its planes after the read) and its MFMAs:
  // the six products per 32x32 tile
  const int r = lane & 31, h = lane >> 5, sw = a_swz((r >> 2) & 3);
  const unsigned a_lo = (unsigned)((((2 * h) ^ sw) * 16)), a_hi = (unsigned)((((2 * h + 1) ^ sw) * 16));
  struct Frags {
    floatx4 raw[T::TM][2];  // A fragment as read (fp32 k = 8h .. 8h + 7)
    bf16x8 a[T::TM][3], b[T::TN][3];
  };
  // fragments of k-step `ks` of the stage in slot `buf`
  auto read_frags = [&](int buf, int ks, Frags& f) __attribute__((always_inline)) {
    if constexpr (T::DBG & 8) return;
    const unsigned char* st = lds + buf * T::STAGE;
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm) {
      const unsigned char* ar = st + ks * T::A_SUB + (wm * T::WM + tm * 32 + r) * 64;
      f.raw[tm][0] = *reinterpret_cast<const floatx4*>(ar + a_lo);
      f.raw[tm][1] = *reinterpret_cast<const floatx4*>(ar + a_hi);
    }
    const unsigned char* bs = st + T::KS * T::A_SUB + ks * T::B_SUB + lane * 16;
#pragma unroll
    for (int tn = 0; tn < T::TN; ++tn)
#pragma unroll
      for (int p = 0; p < 3; ++p)
        f.b[tn][p] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uintx4*>(bs + ((wn * T::TN + tn) * 3 + p) * 1024));
  };
  auto split_frags = [&](Frags& f) __attribute__((always_inline)) {
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm) {
      if constexpr (T::DBG & 2) {
        f.a[tm][0] = __builtin_bit_cast(bf16x8, f.raw[tm][0]);
        f.a[tm][1] = __builtin_bit_cast(bf16x8, f.raw[tm][1]);
        f.a[tm][2] = f.a[tm][0];
        continue;
      }
      uint2 pl[3], ph[3];
      split3v(f.raw[tm][0], pl);
      split3v(f.raw[tm][1], ph);
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        uintx4 v;
        v.x = pl[p].x;
        v.y = pl[p].y;
        v.z = ph[p].x;
        v.w = ph[p].y;
        f.a[tm][p] = __builtin_bit_cast(bf16x8, v);
      }
    }
  };
  floatx16 acc[T::TM][T::TN];
  // MFMAs of one k-step; hook(g) after the six products of 32x32 tile g (SPREAD)
  auto mma = [&](const Frags& f, auto&& hook) __attribute__((always_inline)) {
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
      for (int tn = 0; tn < T::TN; ++tn) {
        // smallest terms first (gemm_f32.hpp's x6 order)
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][2], f.b[tn][0], acc[tm][tn], 0, 0, 0);
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][1], f.b[tn][1], acc[tm][tn], 0, 0, 0);
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][0], f.b[tn][2], acc[tm][tn], 0, 0, 0);
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][1], f.b[tn][0], acc[tm][tn], 0, 0, 0);
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][0], f.b[tn][1], acc[tm][tn], 0, 0, 0);
        acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][0], f.b[tn][0], acc[tm][tn], 0, 0, 0);
        hook(tm * T::TN + tn);
      }
  };
  // ---- explicit slot schedule of one k-step (SCHED): MFMA i of the k-step in slot i;
  // before slot 0 the next k-step's A reads; behind the MFMA of slot i: two of the next
  // B fragment reads (first slots), DMA i of the stage (k-step 0), and from slot PS on
  // the split of the next A fragment in pieces of <= 5 VALU (plane p of an x,y or z,w
  // pair: one v_cvt_pk_bf16_f32, then the two exact residual subtractions)
  auto mma_one = [&](const Frags& f, int i) __attribute__((always_inline)) {
    const int g = i / 6, tm = g / T::TN, tn = g % T::TN, term = i % 6;
    // smallest terms first (gemm_f32.hpp's x6 order): a2b0 a1b1 a0b2 a1b0 a0b1 a0b0
    const int pa = term == 0 ? 2 : term == 1 || term == 3 ? 1 : 0;
    const int pb = term == 0 || term >= 3 ? (term == 4 ? 1 : 0) : term == 1 ? 1 : 2;
    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a[tm][pa], f.b[tn][pb], acc[tm][tn], 0, 0, 0);
  };
  auto read_a = [&](int buf, int ks, Frags& f) __attribute__((always_inline)) {
    if constexpr ((T::DBG & 8) || (T::DBG & 512)) {  // no A reads: opaque stale values
#pragma unroll
      for (int tm = 0; tm < T::TM; ++tm) asm volatile("" : "+v"(f.raw[tm][0]), "+v"(f.raw[tm][1]));
      return;
    }
    const unsigned char* st = lds + buf * T::STAGE;
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm) {
      const unsigned char* ar = st + ks * T::A_SUB + (wm * T::WM + tm * 32 + r) * 64;
      f.raw[tm][0] = *reinterpret_cast<const floatx4*>(ar + a_lo);
      f.raw[tm][1] = *reinterpret_cast<const floatx4*>(ar + a_hi);
    }
  };
  auto read_b = [&](int buf, int ks, Frags& f, int q) __attribute__((always_inline)) {  // fragment q = 3 tn + p
    if constexpr ((T::DBG & 8) || (T::DBG & 256)) {  // no B reads: opaque stale values
      asm volatile("" : "+v"(f.b[q / 3][q % 3]));
      return;
    }
    const unsigned char* bs = lds + buf * T::STAGE + T::KS * T::A_SUB + ks * T::B_SUB + lane * 16;
    f.b[q / 3][q % 3] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uintx4*>(bs + ((wn * T::TN) * 3 + q) * 1024));
  };
  unsigned pk[T::TM][2][3][2];
  auto piece = [&](Frags& f, int q) __attribute__((always_inline)) {  // q < 12 TM
    const int tm = q / 12, half = (q / 6) % 2, p = (q % 6) / 2, part = q % 2;
    floatx4& x = f.raw[tm][half];
    unsigned u;
    if (part == 0) {
      u = cvt_pk_bf16(x.x, x.y);
      if (p < 2) {
        x.x -= bf16_lo(u);
        x.y -= bf16_hi(u);
      }
    } else {
      u = cvt_pk_bf16(x.z, x.w);
      if (p < 2) {
        x.z -= bf16_lo(u);
        x.w -= bf16_hi(u);
      }
    }
    // keep the piece in its slot (machine sinking would move it past the DMA branches,
    // towards the use in the next k-step)
    asm volatile("" : "+v"(u), "+v"(x));
    pk[tm][half][p][part] = u;
  };
  auto assemble = [&](Frags& f) __attribute__((always_inline)) {
#pragma unroll
    for (int tm = 0; tm < T::TM; ++tm)
#pragma unroll
      for (int p = 0; p < 3; ++p) {
        uintx4 v;
        v.x = pk[tm][0][p][0];
        v.y = pk[tm][0][p][1];
        v.z = pk[tm][1][p][0];
        v.w = pk[tm][1][p][1];
        f.a[tm][p] = __builtin_bit_cast(bf16x8, v);
        asm volatile("" : "+v"(f.a[tm][p]));  // the split stays in this k-step
      }
  };
  int c_i = 0, c_st = 0;
  auto tile_end = [&]() __attribute__((always_inline)) {
    if (++c_st == nst) {
      c_st = 0;
      int m0, n0;
      coords(c_i, m0, n0);
      if constexpr (!(T::DBG & 4))
        store_wave_tile<EPI, T::TM, T::TN>(acc, m0 + wm * T::WM, n0 + wn * T::WN, M, N, bias, resid, ldr, out, ldo,
                                           lane);
      zero_acc<T>(acc);
      ++c_i;
    }
  };
  // own DMAs landed up to all but the last `stages` stages issued, then everyone's (and
  // every wave is past its reads of the slot the next issue refills)
  auto wait_stages = [&](auto stages) __attribute__((always_inline)) {
    constexpr int n = decltype(stages)::value;
    const int dwi = T::LDR ? wave - T::NW : wave;
    if constexpr (T::DBG & 128) {  // no barrier (races: timing only)
      if (T::REM && dwi >= 0 && dwi < T::REM)
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)" ::"n"(T::CNT_HI * n) : "memory");
      else
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_waitcnt lgkmcnt(0)" ::"n"(T::CNT_LO * n) : "memory");
      return;
    }
    if (T::REM && dwi >= 0 && dwi < T::REM)
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(T::CNT_HI * n) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(T::CNT_LO * n) : "memory");
    // lgkmcnt(0) as the builtin, visible to the compiler's wait-count pass: it then knows
    // the fragment reads of the previous k-step have landed (as inline asm it does not,
    // and waits lgkmcnt(0) in front of the first MFMA - for this k-step's own reads too)
    __builtin_amdgcn_s_waitcnt(0xC07F);
    asm volatile("s_barrier" ::: "memory");
  };
  zero_acc<T>(acc);

  // Stage j's k-steps multiply from registers while the next k-step's fragments (k-step
  // 0 of stage j + 1 after the last) are read and split; stage j + 1 has landed before
  // stage j starts, and stage j + AHEAD is issued into the slot freed last.
  if constexpr (T::LDR) {
    if (wave >= T::NW) {  // loader waves: the ring, one barrier per stage as the compute waves
#pragma unroll
      for (int d = 0; d < T::AHEAD; ++d) issue(d);
      wait_stages(IC<T::AHEAD - 1>{});  // stage 0 landed
      if constexpr (HAND) {
        // (the kernel's comment has the slot plan and the barrier table)
        static_assert(T::AHEAD == 2, "hand-off: the ring two stages ahead");
        for (int j = 0; j + 2 < S; ++j) {
          wait_stages(IC<0>{});      // B(j + 1): stage j + 1 landed
          issue((j + 2) % T::NBUF);  // stage j + 2 <= S - 1
        }
        if (S >= 2) wait_stages(IC<0>{});  // B(S - 1)
        int m0, n0;
        coords(n_tiles - 1, m0, n0);
        LnTileRegs<2 * T::TM, 2 * T::TN> q;
        ln_tile_load(q, resid, ldr, m0 + wm * T::WM, n0 + wn * T::WN, M, lf, lane);
        wait_stages(IC<0>{});  // B(S): vmcnt(0), the last stage and the residual have landed
        const int ts = (S + (cw >> 1)) % T::NBUF;
        ln_tile_write(q, lds + ts * T::STAGE + (cw & 1) * (T::WM * T::WN * 4), lf, lane);
        __builtin_amdgcn_s_waitcnt(0xC07F);       // t is in LDS
        asm volatile("s_barrier" ::: "memory");  // B(S + 1): the hand-off
        return;
      }
      int l_st = 0;
      [[maybe_unused]] int l_i = 0;
      for (int j = 0; j < S; ++j) {
        wait_stages(IC<T::AHEAD - 2>{});  // stage j + 1 landed
        issue((j + T::AHEAD) % T::NBUF);  // stage j + AHEAD
        if constexpr (ATTN) {
          if (++l_st == nst) {  // X(j): the compute waves' exchange barrier of this tile end
            l_st = 0;
            asm volatile("s_barrier" ::: "memory");
          }
        }
        if constexpr (SPLIT) {
          if (++l_st == nst) {  // stage j is a tile's last (the kernel's comment has the plan)
            l_st = 0;
            static_assert(T::AHEAD == 2, "split epilogue: the ring two stages ahead");
            constexpr int MB = 2 * T::TM, NB16 = 2 * T::TN;
            int m0, n0;
            coords(l_i++, m0, n0);
            const int wr0 = m0 + wm * T::WM, wc0 = n0 + wn * T::WN;
            EpiPre<NB16> pre;  // in flight while the compute waves multiply stage j
            epi_pre_load<EPI, MB, NB16>(pre, wr0, wc0, M, N, bias, lf, lane);
            asm volatile("s_barrier" ::: "memory");  // X(j): the handed block rows are in slot j % 3
            const unsigned char* hs = lds + (j % T::NBUF) * T::STAGE + cw * (HS * NB16 * 1024) + lane * 16;
            floatx4 hacc[MB][NB16];  // (rows below MB - HS are never read)
#pragma unroll
            for (int m = 0; m < HS; ++m)
#pragma unroll
              for (int n = 0; n < NB16; ++n)
                hacc[MB - HS + m][n] = *reinterpret_cast<const floatx4*>(hs + (m * NB16 + n) * 1024);
            store_wave_tile16<EPI, MB, NB16, MB - HS, MB, true>(hacc, wr0, wc0, M, N, bias, resid, ldr, out, ldo, lane,
                                                                lf, &pre);
          }
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing re-read DMAs
      return;
    }
  } else {
#pragma unroll
    for (int d = 0; d < T::AHEAD; ++d) issue(d);
  }
  if constexpr (T::M16) {
    // ---- the k-step on v_mfma_f32_16x16x32_bf16 (compute waves; SCHED, loader waves).
    // The wave tile is MB x NB16 16x16 blocks; one step is a whole 32-deep stage: lane
    // (c = lane & 15, kq = lane >> 4) holds k = 8 kq + j of row / column c of a block, i.e.
    // 16-deep sub-stage kq >> 1, half kq & 1 of the fragments the 32x32x16 body reads.
    // Operands are single-buffered and reloaded in place.  Slot i = 36 m + 6 n + t is
    // product t of block (m, n): the step walks the A row blocks (region m = 36 slots)
    // over all B column blocks.  Region m splits, in sub-pieces of <= 2 VALU per slot, A
    // block m - 1 of the NEXT step (block MB - 1 of this step in region 0) out of `raw`,
    // then reads block m of the next step into `raw`; the last region reloads each B
    // fragment of the next step right behind its last product.  Every read of stage
    // j + 1 is issued in iteration j.
    constexpr int MB = 2 * T::TM, NB16 = 2 * T::TN, RS = NB16 * 6, NM16 = MB * RS, NSUB = 28;
    static_assert(RS >= NSUB + 4, "a region holds one block's split and its raw reads");
    const int c = lane & 15, kq = lane >> 4, hq = kq & 1, sw16 = a_swz((c >> 2) & 3);
    const unsigned a_base = (unsigned)((kq >> 1) * T::A_SUB + (wm * T::WM + c) * 64);
    const unsigned a_lo16 = a_base + (unsigned)(((2 * hq) ^ sw16) * 16);
    const unsigned a_hi16 = a_base + (unsigned)(((2 * hq + 1) ^ sw16) * 16);
    const unsigned b_base =
        (unsigned)(T::KS * T::A_SUB + (kq >> 1) * T::B_SUB + wn * T::TN * 3 * 1024 + hq * 512 + c * 16);
    floatx4 acc4[MB][NB16];
    uintx4 au[MB][3];
    bf16x8 bw[NB16][3];
    floatx4 raw[2];  // chunks 2 hq, 2 hq + 1 of the block being split
    auto rd_raw = [&](const unsigned char* st, int m, int half) __attribute__((always_inline)) {
      raw[half] = *reinterpret_cast<const floatx4*>(st + m * 1024 + (half ? a_hi16 : a_lo16));
    };
    auto rd_b = [&](const unsigned char* st, int n, int p) __attribute__((always_inline)) {
      bw[n][p] = __builtin_bit_cast(
          bf16x8, *reinterpret_cast<const uintx4*>(st + b_base + ((n >> 1) * 3 + p) * 1024 + (n & 1) * 256));
    };
    // sub-piece q < NSUB of the split of `raw` into au[m]: per half, planes 0 and 1 of the
    // x,y and z,w pairs as (convert) (residual lo) (residual hi), then plane 2's converts
    auto sub = [&](int m, int q) __attribute__((always_inline)) {
      const int half = q / 14, rq = q % 14;
      const int p = rq < 12 ? rq / 6 : 2, part = rq < 12 ? (rq % 6) / 3 : rq - 12, op = rq < 12 ? rq % 3 : 0;
      floatx4& x = raw[half];
      if (op == 0) {
        unsigned u = cvt_pk_bf16(x[2 * part], x[2 * part + 1]);
        asm volatile("" : "+v"(u));
        au[m][p][2 * half + part] = u;
      } else {
        const unsigned u = au[m][p][2 * half + part];
        if (op == 1)
          x[2 * part] -= bf16_lo(u);
        else
          x[2 * part + 1] -= bf16_hi(u);
        asm volatile("" : "+v"(x));
      }
    };
    auto zero4 = [&]() __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < MB; ++m)
#pragma unroll
        for (int n = 0; n < NB16; ++n) acc4[m][n] = floatx4{0.f, 0.f, 0.f, 0.f};
    };
    zero4();
    wait_stages(IC<T::AHEAD - 1>{});  // stage 0 landed
    // the operands of a stage whole: A blocks read and split (the last left in `raw`), B read
    auto load_ops = [&](const unsigned char* st) __attribute__((always_inline)) {
#pragma unroll
      for (int m = 0; m < MB; ++m) {
        rd_raw(st, m, 0);
        rd_raw(st, m, 1);
        if (m < MB - 1) {
#pragma unroll
          for (int q = 0; q < NSUB; ++q) sub(m, q);
        }
      }
#pragma unroll
      for (int n = 0; n < NB16; ++n)
#pragma unroll
        for (int p = 0; p < 3; ++p) rd_b(st, n, p);
    };
    load_ops(lds);
    int rb = 1 % T::NBUF;          // ring slot of stage j + 1
    int ib = T::AHEAD % T::NBUF;   // ring slot stage j + AHEAD goes to (8-wave tiles)
    for (int j = 0; j < S; ++j) {
      // stage j + 1 landed.  DEEP: stage j's slot is refilled next, and this wave's reads
      // of it (previous iteration) must have returned; else the slot refilled is stage
      // j - 1's, whose fragments have been multiplied.
      if constexpr (!T::LDR) {
        wait_stages(IC<T::AHEAD - 2>{});
      } else {
        if constexpr (T::DEEP) __builtin_amdgcn_s_waitcnt(0xC07F);
        if constexpr (ATTN || SPLIT) {  // a tile's last stage: its slot is the epilogue's, no read of it may be in flight
          if (c_st == nst - 1) __builtin_amdgcn_s_waitcnt(0xC07F);
        }
        asm volatile("s_barrier" ::: "memory");
      }
      // (HAND, last iteration: slot rb = S % 3 holds no stage - the loader waves are writing t
      // into it while these reads of "stage S" run.  The race is benign only because what the
      // reads return is never multiplied: raw, au and bw are dead after this iteration and
      // must stay so)
      const unsigned char* st = lds + rb * T::STAGE;
      static_for<NM16>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        constexpr int m = i / RS, w = i % RS, n = w / 6, term = w % 6;
        // smallest terms first (gemm_f32.hpp's x6 order): a2b0 a1b1 a0b2 a1b0 a0b1 a0b0
        constexpr int pa = term == 0 ? 2 : term == 1 || term == 3 ? 1 : 0;
        constexpr int pb = term == 0 || term >= 3 ? (term == 4 ? 1 : 0) : term == 1 ? 1 : 2;
        acc4[m][n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, au[m][pa]), bw[n][pb],
                                                             acc4[m][n], 0, 0, 0);
        if constexpr (w >= 2 && w < 2 + NSUB) sub((m + MB - 1) % MB, w - 2);
        if constexpr (w == 2 + NSUB || w == 3 + NSUB) rd_raw(st, m, w - 2 - NSUB);
        if constexpr (m == MB - 1 && term == 2) rd_b(st, n, 2);
        if constexpr (m == MB - 1 && term == 4) rd_b(st, n, 1);
        if constexpr (m == MB - 1 && term == 5) rd_b(st, n, 0);
        if constexpr (!T::LDR && i % T::DSTEP == 0 && i / T::DSTEP < T::CNT_HI) issue_one(ib, i / T::DSTEP);
        __builtin_amdgcn_sched_barrier(0);
      });
      if constexpr (!T::LDR) {
        advance();
        ib = ib + 1 == T::NBUF ? 0 : ib + 1;
      }
      rb = rb + 1 == T::NBUF ? 0 : rb + 1;
      if (++c_st == nst) {
        if constexpr (HAND) {
          if (j == S - 1) break;  // the workgroup's last tile: finished below, from LDS
        }
        c_st = 0;
        int m0, n0;
        coords(c_i, m0, n0);
        if constexpr (ATTN) {
          unsigned char* fs = lds + (j % T::NBUF) * T::STAGE;  // stage j's slot: free until B(j + 2)
          attn_wave_tile<EPI == EPI_ATTN_LNFOLD>(acc4, m0 + wm * T::WM, n0 / T::BN, wn, M, N / 3, bias, lf, at.mask,
                                                 at.scale, out, lane, fs + cw * kAttnStage,
                                                 fs + (cw ^ 1) * kAttnStage);
          // stage j + 1 again: its prefetched copies died above.  Unconditional, so that no path
          // carries them across the epilogue (after the last tile the values are never used)
          load_ops(st);
        } else if constexpr (SPLIT) {
          // the last HS block rows to the SIMD partner, through stage j's slot (free until B(j + 2))
          unsigned char* hs = lds + (j % T::NBUF) * T::STAGE + cw * (HS * NB16 * 1024) + lane * 16;
#pragma unroll
          for (int m = 0; m < HS; ++m)
#pragma unroll
            for (int n = 0; n < NB16; ++n)
              *reinterpret_cast<floatx4*>(hs + (m * NB16 + n) * 1024) = acc4[MB - HS + m][n];
          __builtin_amdgcn_s_waitcnt(0xC07F);       // they are in LDS
          asm volatile("s_barrier" ::: "memory");  // X(j)
          // (its own loads stay behind the barrier: issued in front of it, the row statistics' 16 load
          // registers beside the accumulators and the next stage's operands spill 7 - 9 VGPRs)
          store_wave_tile16<EPI, MB, NB16, 0, MB - HS>(acc4, m0 + wm * T::WM, n0 + wn * T::WN, M, N, bias, resid, ldr,
                                                       out, ldo, lane, lf);
        } else {
          store_wave_tile16<EPI, MB, NB16>(acc4, m0 + wm * T::WM, n0 + wn * T::WN, M, N, bias, resid, ldr, out, ldo,
                                           lane, lf);
        }
        zero4();
        ++c_i;
      }
    }
    if constexpr (HAND) {
      asm volatile("s_barrier" ::: "memory");  // B(S + 1): the loader waves have written t
      int m0, n0;
      coords(n_tiles - 1, m0, n0);
      const int ts = (S + (cw >> 1)) % T::NBUF;
      store_wave_tile16_ln_stats<1, MB, NB16, true>(acc4, m0 + wm * T::WM, n0 + wn * T::WN, M, bias, resid, ldr, out,
                                                    ldo, lane, lf,
                                                    lds + ts * T::STAGE + (cw & 1) * (T::WM * T::WN * 4));
      return;
    }
    if constexpr (!T::LDR) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing re-read DMAs
    return;
  }
  wait_stages(IC<T::AHEAD - 1>{});  // stage 0 landed
  Frags f0 = {}, f1 = {};
  read_frags(0, 0, f0);
  split_frags(f0);
  // iteration j with `fa` holding its first k-step's fragments
  auto step = [&](int j, Frags& fa, Frags& fb) __attribute__((always_inline)) {
    wait_stages(IC<T::AHEAD - 2>{});  // stage j + 1 landed
    const int buf = (j + T::AHEAD) % T::NBUF;  // stage j + AHEAD goes here
    if constexpr (!T::SCHED && !T::LDR) issue(buf);
    static_for<T::KS>([&](auto kc) {
      constexpr int ks = decltype(kc)::value;
      Frags& cur = ks % 2 == 0 ? fa : fb;
      Frags& nxt = ks % 2 == 0 ? fb : fa;
      if constexpr (T::SCHED) {
        constexpr int NM = T::TM * T::TN * 6, NBR = 3 * T::TN, PS = T::PS, NP = 12 * T::TM;
        constexpr int PER = (NP + (NM - PS) - 1) / (NM - PS);
        const int rbuf = ks + 1 < T::KS ? j % T::NBUF : (j + 1) % T::NBUF;
        constexpr int rks = ks + 1 < T::KS ? ks + 1 : 0;
        read_a(rbuf, rks, nxt);
        __builtin_amdgcn_sched_barrier(0);
        static_for<NM>([&](auto ic) {
          constexpr int i = decltype(ic)::value;
          mma_one(cur, i);
          constexpr bool dma_slot = !T::LDR && ks == 0 && i % T::DSTEP == 0 && i / T::DSTEP < T::CNT_HI;
          // B read pair index of slot i: slots from BR0 on that carry no DMA
          constexpr int bslot = [] {
            int n = 0;
            for (int k = T::BR0; k < i; ++k)
              if (!(!T::LDR && ks == 0 && k % T::DSTEP == 0 && k / T::DSTEP < T::CNT_HI) || T::DSTEP == 1) ++n;
            return n;
          }();
          if constexpr (i >= T::BR0 && (!dma_slot || T::DSTEP == 1)) {
            if constexpr (2 * bslot < NBR) read_b(rbuf, rks, nxt, 2 * bslot);
            if constexpr (2 * bslot + 1 < NBR) read_b(rbuf, rks, nxt, 2 * bslot + 1);
          }
          if constexpr (dma_slot) issue_one(buf, i / T::DSTEP);
          if constexpr (i >= PS) {
            static_for<PER>([&](auto pc) {
              constexpr int q = (i - PS) * PER + decltype(pc)::value;
              if constexpr (q < NP) piece(nxt, q);
            });
          }
          __builtin_amdgcn_sched_barrier(0);
        });
        assemble(nxt);
      } else {
        if constexpr (ks + 1 < T::KS)
          read_frags(j % T::NBUF, ks + 1, nxt);
        else
          read_frags((j + 1) % T::NBUF, 0, nxt);
        mma(cur, [](int) {});
        split_frags(nxt);
      }
    });
    if constexpr (T::SCHED && !T::LDR) advance();
    tile_end();
  };
  if constexpr (T::KS % 2 == 0) {
    for (int j = 0; j < S; ++j) step(j, f0, f1);
  } else {
    for (int j = 0; j < S; j += 2) {
      step(j, f0, f1);
      if (j + 1 >= S) break;
      step(j + 1, f1, f0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the trailing re-read DMAs
}

// EPI_ATTN_*'s attention from a stored qkv (launch_attn32): one workgroup of 4 waves per (128
// rows, head), wave (wm, wn) loading the accumulator image the fused kernel's compute wave (wm,
// wn) holds at its tile end - block (m, n), register e of lane (c, g) = row 16 m + 4 g + e, column
// 16 (n & 1) + c of Q | K | V (n >> 1) for head dims 32 wn .. + 31 - rows past M clamped, as the
// fused kernel's A loads are.
__global__ __launch_bounds__(256) void attn32_kernel(const float* __restrict__ qkv, const int* __restrict__ mask,
                                                     float* __restrict__ ctx, int M, int H, float scale) {
  __shared__ __attribute__((aligned(16))) unsigned char stg[4 * kAttnStage];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int cw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wm = cw >> 1, wn = cw & 1;
  const int heads = H / 64, head = blockIdx.x % heads, wr0 = (blockIdx.x / heads) * 128 + 64 * wm;
  floatx4 acc[4][6];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float* row = qkv + (int64_t)min(wr0 + 16 * m + 4 * g + e, M - 1) * (3 * H) + 64 * head + 32 * wn + c;
#pragma unroll
      for (int n = 0; n < 6; ++n) acc[m][n][e] = row[(n >> 1) * H + 16 * (n & 1)];
    }
  attn_wave_tile<false, true>(acc, wr0, head, wn, M, H, nullptr, LnFold{}, mask, scale, ctx, lane,
                              stg + cw * kAttnStage, stg + (cw ^ 1) * kAttnStage);
}

// W [N][K] fp32 -> W3: one thread per (row n < Np, 8-wide k chunk); rows past N are zero.
__global__ __launch_bounds__(256) void split_w3_kernel(const float* __restrict__ W, int N, int K,
                                                       uintx4* __restrict__ w3) {
  const int k8n = K >> 3, np = (N + 31) & ~31;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)np * k8n) return;
  const int n = (int)(idx / k8n), k8 = (int)(idx - (int64_t)n * k8n);
  floatx4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
  if (n < N) {
    lo = *reinterpret_cast<const floatx4*>(W + (int64_t)n * K + 8 * k8);
    hi = *reinterpret_cast<const floatx4*>(W + (int64_t)n * K + 8 * k8 + 4);
  }
  uint2 pl[3], ph[3];
  split3(lo, pl);
  split3(hi, ph);
  const int kb = k8 >> 1, hh = k8 & 1, nb = n >> 5, rr = n & 31;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    uintx4 v;
    v.x = pl[p].x;
    v.y = pl[p].y;
    v.z = ph[p].x;
    v.w = ph[p].y;
    w3[((int64_t)(nb * (K >> 4) + kb) * 3 + p) * 64 + hh * 32 + rr] = v;
  }
}

// Product tiles (mq_debug_gemm_x6p tile codes 0-3, 7), all on the M16 k-step
// (v_mfma_f32_16x16x32_bf16, 32-deep stages).  Measured at M = 8192 (BERT-base batched
// shapes, tools/gemm_x6p_bench.py --ab, profiles/mfma16/gemm_ab.jsonl): the loader-wave
// 128 x 192 tile runs QKV / out-proj / FFN-up / FFN-down at 240 / 207 / 221 / 251 TF
// fp32-equivalent (215 / 180 / 203 / 217 on the 32x32x16 k-step, tile 16, same process).
using X6p0 = X6pTile<2, 2, 2, 3, 3, 2, 4, true, 0, 1, 0, 6, true, true>;         // 128 x 192, 4 compute + 4 loader waves
using X6p1 = X6pTile<4, 1, 2, 3, 3, 2, 4, true, 0, 1, 0, 6, true, true>;         // 256 x 96, same
using X6p2 = X6pTile<4, 2, 1, 3, 3, 2, 4, true, 0, 2, 1, 6, false, true>;        // 128 x 192, 8 waves, DMAs from 0-3
using X6p3 = X6pTile<4, 2, 2, 3, 2, 2, 8, true, 0, 6, 1, 8, false, true, true>;  // 256 x 192, 8 waves, 2 slots
// measurement variants (tile codes 4-6; 7 is a product tile): the ring 3 stages ahead
using X6p4 = X6pTile<2, 2, 2, 3, 3, 2, 4, true, 0, 1, 0, 6, true, true, true>;   // tile 0
using X6p5 = X6pTile<2, 2, 1, 3, 3, 2, 4, true, 0, 1, 0, 6, true, true, true>;   // tile 7
using X6p6 = X6pTile<4, 1, 2, 3, 3, 2, 4, true, 0, 1, 0, 6, true, true, true>;   // tile 1
using X6p7 = X6pTile<2, 2, 1, 3, 3, 2, 4, true, 0, 1, 0, 6, true, true>;         // 64 x 192, loaders
// tile codes 16 / 17: the former k-step of tiles 0 / 7 (v_mfma_f32_32x32x16_bf16, 16-deep
// stages, 4 slots), kept to re-measure the two MFMA shapes in one library.  Same split and
// products in the same order but 16 k per MFMA: fp32-class, NOT bit-identical to the others.
using X6p16 = X6pTile<2, 2, 2, 3, 4, 1, 4, true, 0, 1, 0, 6, true>;
using X6p17 = X6pTile<2, 2, 1, 3, 4, 1, 4, true, 0, 1, 0, 6, true>;

template <class T, int EPI, bool FORMER = false>
void launch_t(const X6pArgs& g, int num_cus, hipStream_t s) {
  // stage depth must divide K: else the 16-deep 8-wave tile (32x32x16 arithmetic).  No caller
  // gets here: launch_gemm's K is a multiple of kBK = 32, as mq_debug_gemm_x6p's.
  if constexpr (EPI < EPI_RESID_LN_STATS) {
    if (g.K % (16 * T::KS) != 0) {
      launch_t<X6pTile<4, 2, 1, 3, 4>, EPI>(g, num_cus, s);
      return;
    }
  }
  const int tiles = ((g.M + T::BM - 1) / T::BM) * ((g.N + T::BN - 1) / T::BN);
  int grid = (std::min(tiles, num_cus) + 7) / 8 * 8;  // one workgroup per CU, a multiple of 8
  if (g.max_wg > 0) grid = std::min(grid, g.max_wg);
  const int tiles_m = (g.M + T::BM - 1) / T::BM, tiles_n = (g.N + T::BN - 1) / T::BN;
  int rx = g.rx;
  if (rx < 0) rx = region_pick_rx(tiles_m, tiles_n, (double)T::BM * g.K * 4, (double)T::BN * g.K * 6, grid);
  if (rx > 0 && (8 % rx != 0 || rx > tiles_n || 8 / rx > tiles_m || grid < 8)) rx = 0;  // (a region per XCD)
  hipLaunchKernelGGL((gemm_x6p_kernel<T, EPI, FORMER>), dim3(grid), dim3(T::THREADS), 0, s, g.A, g.lda,
                     static_cast<const unsigned char*>(g.W3), g.bias, g.resid, g.ldr, g.out, g.ldo, g.M, g.N, g.K, rx,
                     g.lf, g.at);
}

template <int EPI>
void launch_tile(const X6pArgs& g, int tile, int num_cus, hipStream_t s) {
#ifdef MQ_X6P_DBG
  if (tile >= 8) {  // measurement builds: tiles 1 / 0 minus parts (X6pTile DBG bits)
    switch (tile) {
      case 8: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 64, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      case 9: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 66, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      case 10: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 8, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      case 11: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 74, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      case 12: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 2, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      case 13: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 256, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      case 14: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 512, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
      default: launch_t<X6pTile<2, 2, 2, 3, 4, 1, 4, true, 128, 1, 0, 6, true>, EPI>(g, num_cus, s); return;
    }
  }
#endif
  switch (tile) {
    case 1: launch_t<X6p1, EPI>(g, num_cus, s); return;
    case 2: launch_t<X6p2, EPI>(g, num_cus, s); return;
    case 3: launch_t<X6p3, EPI>(g, num_cus, s); return;
    case 4: launch_t<X6p4, EPI>(g, num_cus, s); return;
    case 5: launch_t<X6p5, EPI>(g, num_cus, s); return;
    case 6: launch_t<X6p6, EPI>(g, num_cus, s); return;
    case 7: launch_t<X6p7, EPI>(g, num_cus, s); return;
    case 16: launch_t<X6p16, EPI>(g, num_cus, s); return;
    case 17: launch_t<X6p17, EPI>(g, num_cus, s); return;
    // 20 / 21: tiles 0 / 1 with the former epilogue (kinds that have one form run as 0 / 1)
    case 20: launch_t<X6p0, EPI, epi_is_split(EPI)>(g, num_cus, s); return;
    case 21: launch_t<X6p1, EPI, epi_is_split(EPI)>(g, num_cus, s); return;
    default: launch_t<X6p0, EPI>(g, num_cus, s); return;
  }
}

// the LayerNorm-fold epilogues: the default tiles only; 20 / 21 = tiles 0 / 1 with the former
// epilogue (the producer without its hand-off, the GELU consumers without the split)
template <int EPI>
void launch_tile_fold(const X6pArgs& g, int tile, int num_cus, hipStream_t s) {
  constexpr bool HAS_FORMER = EPI == EPI_RESID_LN_STATS || epi_is_split(EPI);
  switch (tile) {
    case 1: launch_t<X6p1, EPI>(g, num_cus, s); return;
    case 20: launch_t<X6p0, EPI, HAS_FORMER>(g, num_cus, s); return;
    case 21: launch_t<X6p1, EPI, HAS_FORMER>(g, num_cus, s); return;
    default: launch_t<X6p0, EPI>(g, num_cus, s); return;
  }
}

// one wave per weight row n: Wg[n][:] = g * W[n][:], s[n] and c[n] summed in float64
__global__ __launch_bounds__(256) void ln_fold_weight_kernel(const float* __restrict__ W,
                                                             const float* __restrict__ bias,
                                                             const float* __restrict__ g,
                                                             const float* __restrict__ b, int N, int K,
                                                             float* __restrict__ Wg, float* __restrict__ s_out,
                                                             float* __restrict__ c_out) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  double sg = 0.0, sb = 0.0;
  for (int k = lane; k < K; k += 64) {
    const float w = W[(int64_t)n * K + k];
    const float wg = g[k] * w;
    Wg[(int64_t)n * K + k] = wg;
    sg += (double)wg;
    sb += (double)b[k] * (double)w;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sg += __shfl_xor(sg, off);
    sb += __shfl_xor(sb, off);
  }
  if (lane == 0) {
    s_out[n] = (float)sg;
    c_out[n] = (float)((double)bias[n] + sb);
  }
}

}  // namespace

void launch_ln_fold_weight(const float* W, const float* bias, const float* g, const float* b, int N, int K, float* Wg,
                           float* s_out, float* c_out, hipStream_t s) {
  hipLaunchKernelGGL(ln_fold_weight_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, W, bias, g, b, N, K, Wg,
                     s_out, c_out);
}

void launch_attn32(const float* qkv, const int* mask, float* ctx, int M, int H, float scale, hipStream_t s) {
  hipLaunchKernelGGL(attn32_kernel, dim3((unsigned)(((M + 127) / 128) * (H / 64))), dim3(256), 0, s, qkv, mask, ctx, M,
                     H, scale);
}

void launch_split_w3(const float* W, int N, int K, void* w3, hipStream_t s) {
  const int64_t n = (int64_t)((N + 31) & ~31) * (K >> 3);
  hipLaunchKernelGGL(split_w3_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, W, N, K,
                     static_cast<uintx4*>(w3));
}

int x6p_pick_tile(int M, int N, int num_cus) {
  // tiles 0 (128 x 192) and 1 (256 x 96) cover the same area at the same measured rate:
  // fewer rounds wins, 128 x 192 on a tie (M = 8192 at N = 768 / 1536 / 2304 / 3072 runs
  // whole rounds of 256 tiles on it)
  auto rounds = [&](int bm, int bn) {
    const int64_t tiles = (int64_t)((M + bm - 1) / bm) * ((N + bn - 1) / bn);
    return (tiles + num_cus - 1) / num_cus;
  };
  return rounds(256, 96) < rounds(128, 192) ? 1 : 0;
}

void launch_gemm_x6p(const X6pArgs& g, int epi, int tile, int num_cus, hipStream_t s) {
  if (tile < 0) {
    // (out-proj, N = K = 768 at M = 8192, ran 64 x 192 tiles two per CU on the 32x32x16
    // k-step; on the 16x16x32 one 128 x 192 is the faster there too: 46.8 vs 50.0 / 51.6 us,
    // profiles/mfma16/gemm_ab.jsonl)
    tile = x6p_pick_tile(g.M, g.N, num_cus);
  }
  // MQ_ENC_OPT_EPI_SPLIT 0: the single-wave consumer epilogue (the producer keeps its hand-off)
  if (g.former_epi && epi_is_split(epi) && (tile == 0 || tile == 1)) tile += 20;
  switch (epi) {
    case EPI_GELU_ERF: launch_tile<EPI_GELU_ERF>(g, tile, num_cus, s); return;
    case EPI_GELU_TANH: launch_tile<EPI_GELU_TANH>(g, tile, num_cus, s); return;
    case EPI_RESID: launch_tile<EPI_RESID>(g, tile, num_cus, s); return;
    case EPI_RESID_LN_STATS: launch_tile_fold<EPI_RESID_LN_STATS>(g, tile, num_cus, s); return;
    case EPI_BIAS_LNFOLD: launch_tile_fold<EPI_BIAS_LNFOLD>(g, tile, num_cus, s); return;
    case EPI_GELU_ERF_LNFOLD: launch_tile_fold<EPI_GELU_ERF_LNFOLD>(g, tile, num_cus, s); return;
    case EPI_GELU_TANH_LNFOLD: launch_tile_fold<EPI_GELU_TANH_LNFOLD>(g, tile, num_cus, s); return;
    case EPI_ATTN_BIAS: launch_t<X6p0, EPI_ATTN_BIAS>(g, num_cus, s); return;
    case EPI_ATTN_LNFOLD: launch_t<X6p0, EPI_ATTN_LNFOLD>(g, num_cus, s); return;
    default: launch_tile<EPI_BIAS>(g, tile, num_cus, s); return;
  }
}

}  // namespace mq

extern "C" {

// Test / measurement hooks (include/mq.h).
int64_t mq_debug_w3_bytes(int N, int K) { return N > 0 && K > 0 && K % 16 == 0 ? (int64_t)mq::w3_bytes(N, K) : -1; }

int mq_debug_split_w3(const float* W, int N, int K, void* w3, void* stream) {
  using namespace mq;
  clear_error();
  MQ_CHECK_ARG(W && w3, "NULL buffer");
  MQ_CHECK_ARG(N > 0 && K > 0 && K % 16 == 0, "bad shape N=%d K=%d", N, K);
  launch_split_w3(W, N, K, w3, (hipStream_t)stream);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_gemm_x6p(const float* A, const void* W3, const float* bias, const float* resid, float* out, int M,
                      int N, int K, int epi, int tile, void* stream) {
  using namespace mq;
  clear_error();
  MQ_CHECK_ARG(A && W3 && bias && out && (epi != EPI_RESID || resid), "NULL buffer");
  MQ_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 32 == 0, "bad shape M=%d N=%d K=%d", M, N, K);
  // tile codes >= 100: tile code % 100 with the region split rx = code / 100 - 1 (0 = the
  // plain walk); below 100 the automatic pick
  const int rx = tile >= 100 ? tile / 100 - 1 : -1;
  if (tile >= 100) tile %= 100;
  MQ_CHECK_ARG(epi >= 0 && epi <= 3 && tile >= -1 && (tile <= 17 || tile == 20 || tile == 21) && rx <= 8,
               "bad epi/tile");
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  X6pArgs g{A, K, W3, bias, resid, N, out, N, M, N, K};
  g.rx = rx;
  launch_gemm_x6p(g, epi, tile, cus, (hipStream_t)stream);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_ln_fold_weight(const float* W, const float* bias, const float* g, const float* b, int N, int K,
                            float* Wg, float* s_out, float* c_out, void* stream) {
  using namespace mq;
  clear_error();
  MQ_CHECK_ARG(W && bias && g && b && Wg && s_out && c_out, "NULL buffer");
  MQ_CHECK_ARG(N > 0 && K > 0, "bad shape N=%d K=%d", N, K);
  launch_ln_fold_weight(W, bias, g, b, N, K, Wg, s_out, c_out, (hipStream_t)stream);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_gemm_x6p_ln(const float* A, const void* W3, const float* bias, const float* resid, float* out, int M,
                         int N, int K, int epi, int tile, const float* stats_in, float* stats_out, const float* g,
                         const float* b, const float* s_fold, float eps, void* stream) {
  using namespace mq;
  clear_error();
  MQ_CHECK_ARG(A && W3 && bias && out, "NULL buffer");
  MQ_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 32 == 0, "bad shape M=%d N=%d K=%d", M, N, K);
  MQ_CHECK_ARG((tile >= -1 && tile <= 1) || tile == 20 || tile == 21,
               "the LayerNorm-fold epilogues run on tiles 0 and 1 (20 / 21: their former epilogues; got %d)", tile);
  if (epi == EPI_RESID_LN_STATS) {
    MQ_CHECK_ARG(resid && stats_out && (!stats_in || (g && b)), "producer: NULL buffer");
    MQ_CHECK_ARG(N == kLnPartW * kLnMaxParts, "producer: N must be %d (got %d)", kLnPartW * kLnMaxParts, N);
    MQ_CHECK_ARG((int64_t)M * N < (1ll << 29), "producer: M * N must stay below 2^29 (32-bit byte offsets)");
  } else {
    MQ_CHECK_ARG(epi_is_lnfold(epi), "epi must be a LayerNorm-fold kind (got %d)", epi);
    MQ_CHECK_ARG(stats_in && s_fold, "consumer: NULL buffer");
    // (the encoder's consumers run at K = 768, the width the partials describe; the epilogue's
    // arithmetic takes the [M][8] partials as they are at any K)
  }
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  X6pArgs a{A, K, W3, bias, resid, N, out, N, M, N, K};
  a.lf.stats_in = stats_in;
  a.lf.stats_out = stats_out;
  a.lf.g = g;
  a.lf.b = b;
  a.lf.s = s_fold;
  a.lf.eps = eps;
  launch_gemm_x6p(a, epi, tile, cus, (hipStream_t)stream);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

int mq_debug_gemm_x6p_attn(const float* A, const void* W3, const float* bias, const int* mask, float* ctx, int M,
                           int K, int heads, float scale, int epi, const float* stats_in, const float* s_fold,
                           float eps, int max_workgroups, void* stream) {
  using namespace mq;
  clear_error();
  MQ_CHECK_ARG(A && W3 && bias && mask && ctx, "NULL buffer");
  MQ_CHECK_ARG(M > 0 && M % 32 == 0 && K > 0 && K % 32 == 0 && heads > 0 && heads <= 1024,
               "bad shape M=%d K=%d heads=%d (M and K must be multiples of 32)", M, K, heads);
  MQ_CHECK_ARG((int64_t)M * heads * 64 < (1ll << 31) && (int64_t)M * K < (1ll << 29), "M too large");
  MQ_CHECK_ARG(epi == EPI_ATTN_BIAS || epi == EPI_ATTN_LNFOLD, "epi must be an attention kind (got %d)", epi);
  MQ_CHECK_ARG(epi != EPI_ATTN_LNFOLD || (stats_in && s_fold), "fold: NULL buffer");
  MQ_CHECK_ARG(max_workgroups >= 0 && max_workgroups % 8 == 0,
               "max_workgroups must be 0 or a multiple of 8 (got %d)", max_workgroups);
  int dev = 0, cus = 256;
  (void)hipGetDevice(&dev);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  const int H = 64 * heads;
  X6pArgs a{A, K, W3, bias, nullptr, 0, ctx, H, M, 3 * H, K};
  a.lf.stats_in = stats_in;
  a.lf.s = s_fold;
  a.lf.eps = eps;
  a.at.mask = mask;
  a.at.scale = scale;
  a.max_wg = max_workgroups;
  launch_gemm_x6p(a, epi, 0, cus, (hipStream_t)stream);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}

}  // extern "C"
