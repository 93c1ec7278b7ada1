// docmask.hip - document-text row masks (Chroma's where_document {"$contains": s}) for the
// filtered searches: mq_mask_contains scans the store's device text mirror for a byte
// pattern and writes the rows that hold it into a row bitmask (K12).
//
// contains_scan_kernel is position-parallel over the blob, not one row per thread (row
// lengths are skewed).  One 256-thread workgroup owns a span of MQ_CONTAINS_SPAN_BYTES text
// bytes: it stages the span plus a halo of pattern_len - 1 bytes into LDS with 16-byte loads
// (the loads that would cross text_bytes are done byte by byte: nothing behind the blob is
// read), and each lane tests the 16 start positions of each of its 16-byte chunks against the
// pattern's first <= 4 bytes held in a register; only a position that passes is verified
// against the rest of the pattern, from LDS.  A hit at byte p belongs to the row r with
// offsets[r] <= p < offsets[r + 1] and counts only if p + pattern_len <= offsets[r + 1] (a
// match never spans two rows).  The span's row ends are staged in LDS once (the first and
// last row of the span by two wave-wide 64-ary searches of offsets); a lane finds the row of
// its first hit by a binary search of those and walks forward from there.  Hits are OR-ed into an
// LDS bitmap of the span's rows and flushed with one vector atomic per non-zero word into the
// caller's scratch hit mask; contains_finish_kernel then applies negate, the tail and the
// mode.  The result does not depend on the order of the atomics.
#include <cstring>

#include "common.hpp"

namespace {

using namespace mq;

constexpr int kSpan = MQ_CONTAINS_SPAN_BYTES;
constexpr int kThreads = 256;
constexpr int kChunks = kSpan / 16;                 // 16-byte chunks of start positions per span
constexpr int kChunksPerThread = kChunks / kThreads;
constexpr int kHaloChunks = MQ_CONTAINS_MAX_BYTES / 16;
constexpr int kRowCap = 2048;                       // row ends / hit bits of a span kept in LDS
constexpr int kHitWords = kRowCap / 32 + 1;         // + 1: the span's first row starts mid-word
static_assert(kChunks % kThreads == 0, "a span is a whole number of chunks per thread");

struct PatWords {
  unsigned w[MQ_CONTAINS_MAX_BYTES / 4];
};

// 16 bytes of text at byte offset b (a multiple of 16; text is 16-byte aligned); bytes at or
// past text_bytes read as 0 and are never loaded
__device__ __forceinline__ uint4 load16(const unsigned char* __restrict__ text, int64_t b, int64_t text_bytes) {
  if (b + 16 <= text_bytes) return *reinterpret_cast<const uint4*>(text + b);
  unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    unsigned v = 0;
    if (b + j < text_bytes) v = text[b + j];
    v <<= 8 * (j & 3);
    if (j < 4) w0 |= v;
    else if (j < 8) w1 |= v;
    else if (j < 12) w2 |= v;
    else w3 |= v;
  }
  return make_uint4(w0, w1, w2, w3);
}

// the row holding byte p: the first r in [0, n) with offsets[r + 1] > p (zero-length rows
// are skipped); n - 1 if there is none, so the result is a row whatever offsets holds
// One whole wave searches: each step its 64 lanes probe 64 evenly spaced rows of the candidate
// range and a ballot narrows it 64-fold, so 1M rows take 4 dependent loads, not 20 (a one-lane
// binary search of offsets per span kept the other waves at the barrier: +40 % scan time).
__device__ __forceinline__ int64_t row_of(const int64_t* __restrict__ offsets, int64_t n, int64_t p, int lane) {
  int64_t lo = 0, len = n;  // the answer is in [lo, lo + len)
  while (len > 1) {
    const int64_t step = (len + 63) >> 6, last = lo + len - 1;
    int64_t r = lo + (lane + 1) * step - 1;  // lane's probe; the last lanes share the range's last row
    if (r > last) r = last;
    const unsigned long long b = __ballot(offsets[r + 1] > p);
    if (b == 0) return last;  // no row ends after p
    const int f = __ffsll((long long)b) - 1;  // the answer lies in lane f's stretch
    lo += f * step;
    len = (lo + step - 1 > last ? last : lo + step - 1) - lo + 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void contains_scan_kernel(const unsigned char* __restrict__ text,
                                                                 int64_t text_bytes,
                                                                 const int64_t* __restrict__ offsets, int64_t n,
                                                                 PatWords pat, int m, unsigned* __restrict__ hits) {
  __shared__ __attribute__((aligned(16))) unsigned char s_text[kSpan + 16 * kHaloChunks];
  __shared__ __attribute__((aligned(16))) unsigned s_pat[MQ_CONTAINS_MAX_BYTES / 4];
  __shared__ unsigned s_end[kRowCap];  // end of the span's row i, relative to the span's first byte
  __shared__ unsigned s_hit[kHitWords];
  __shared__ int64_t s_rows[2];

  const int tid = threadIdx.x;
  const int64_t span0 = (int64_t)blockIdx.x * kSpan;  // < text_bytes by the grid

  uint4 v[kChunksPerThread];
#pragma unroll
  for (int j = 0; j < kChunksPerThread; ++j)
    v[j] = load16(text, span0 + (int64_t)(tid + j * kThreads) * 16, text_bytes);
  const int halo_chunks = (m - 1 + 15) / 16 > 1 ? (m - 1 + 15) / 16 : 1;
  uint4 h = make_uint4(0, 0, 0, 0);
  if (tid < halo_chunks) h = load16(text, span0 + kSpan + (int64_t)tid * 16, text_bytes);
  if (tid < 2 * kWave) {  // wave 0: the row of the span's first byte, wave 1: of its last
    const int64_t last = (span0 + kSpan < text_bytes ? span0 + kSpan : text_bytes) - 1;
    const int64_t r = row_of(offsets, n, tid < kWave ? span0 : last, tid & (kWave - 1));
    if ((tid & (kWave - 1)) == 0) s_rows[tid / kWave] = r;
  }
#pragma unroll
  for (int j = 0; j < kChunksPerThread; ++j) *reinterpret_cast<uint4*>(s_text + (tid + j * kThreads) * 16) = v[j];
  if (tid < kHaloChunks) *reinterpret_cast<uint4*>(s_text + kSpan + tid * 16) = h;
  if (tid < MQ_CONTAINS_MAX_BYTES / 4) s_pat[tid] = pat.w[tid];
  if (tid < kHitWords) s_hit[tid] = 0u;
  __syncthreads();

  const int64_t r_lo = s_rows[0], total = s_rows[1] - r_lo + 1;  // the span's rows: r_lo .. r_lo + total - 1
  const int cnt = total < kRowCap ? (int)total : kRowCap;
  auto clamp_end = [&](int64_t row) -> unsigned {
    const int64_t e = offsets[row + 1] - span0;
    return e < 0 ? 0u : e > 0x7fffffff ? 0x7fffffffu : (unsigned)e;
  };
  for (int i = tid; i < cnt; i += kThreads) s_end[i] = clamp_end(r_lo + i);
  __syncthreads();
  // rows past the LDS table (a span of more than kRowCap rows) read offsets
  auto row_end = [&](int64_t i) -> unsigned { return i < cnt ? s_end[i] : clamp_end(r_lo + i); };
  // first i in [lo, total) whose row ends after pos, else total - 1
  auto find_row = [&](int64_t lo, unsigned pos) -> int64_t {
    int64_t hi = total - 1;
    while (lo < hi) {
      const int64_t mid = lo + ((hi - lo) >> 1);
      if (row_end(mid) > pos) hi = mid;
      else lo = mid + 1;
    }
    return lo;
  };

  const unsigned pmask = m >= 4 ? ~0u : (1u << (8 * m)) - 1u;
  const unsigned p0 = pat.w[0] & pmask;
  // start positions (relative to the span) up to lim leave room for the pattern in the blob
  const int64_t room = text_bytes - m - span0;
  const int lim = room >= kSpan ? kSpan - 1 : (int)room;  // may be negative: no position
  const unsigned char* s_patb = reinterpret_cast<const unsigned char*>(s_pat);
  int64_t cur = -1, marked = -1;
#pragma unroll
  for (int j = 0; j < kChunksPerThread; ++j) {
    const int base = (tid + j * kThreads) * 16;
    const uint4 a = *reinterpret_cast<const uint4*>(s_text + base);
    const unsigned nx = *reinterpret_cast<const unsigned*>(s_text + base + 16);
    const unsigned w[5] = {a.x, a.y, a.z, a.w, nx};
    unsigned hm = 0;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
      const unsigned long long pair = ((unsigned long long)w[(s >> 2) + 1] << 32) | w[s >> 2];
      const unsigned word = (unsigned)(pair >> (8 * (s & 3)));
      hm |= ((word & pmask) == p0 ? 1u : 0u) << s;
    }
    const int left = lim - base;  // start positions base .. base + left are inside the blob
    if (left < 15) hm &= left < 0 ? 0u : (2u << left) - 1u;
    while (hm) {
      const int s = __ffs((int)hm) - 1;
      hm &= hm - 1;
      const unsigned pos = (unsigned)(base + s);
      bool ok = true;
      for (int t = 4; t < m; ++t)
        if (s_text[pos + t] != s_patb[t]) {
          ok = false;
          break;
        }
      if (!ok) continue;
      if (cur < 0) {
        cur = find_row(0, pos);
      } else if (row_end(cur) <= pos) {
        if (cur + 1 < total) ++cur;
        if (row_end(cur) <= pos) cur = find_row(cur, pos);
      }
      if (cur == marked || pos + (unsigned)m > row_end(cur)) continue;  // the match would cross the row's end
      marked = cur;
      const int64_t r = r_lo + cur;
      if (cur < cnt) atomicOr(&s_hit[((int)(r_lo & 31) + (int)cur) >> 5], 1u << (r & 31));
      else atomicOr(&hits[r >> 5], 1u << (r & 31));
    }
  }
  __syncthreads();
  if (tid < kHitWords && s_hit[tid]) atomicOr(&hits[(r_lo >> 5) + tid], s_hit[tid]);
}

// bits (mode)= hits ^ negate over rows [0, n): the bits past n in the last word are 0
__global__ __launch_bounds__(256) void contains_finish_kernel(const unsigned* __restrict__ hits, int64_t n,
                                                              int negate, unsigned* __restrict__ bits, int mode) {
  const int64_t w = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (w * 32 >= n) return;
  unsigned x = negate ? ~hits[w] : hits[w];
  const int64_t rem = n - w * 32;
  if (rem < 32) x &= (1u << rem) - 1u;
  bits[w] = mode == MQ_MASK_AND ? (bits[w] & x) : mode == MQ_MASK_OR ? (bits[w] | x) : x;
}

// Device of a pointer (HIP device memory), or -1 (host / unknown).
int pointer_device(const void* p) {
  hipPointerAttribute_t a;
  if (!p || hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return -1;
  }
  return a.type == hipMemoryTypeDevice ? a.device : -1;
}

}  // namespace

extern "C" int mq_mask_contains(const uint8_t* text, int64_t text_bytes, const int64_t* offsets, int64_t n,
                                const uint8_t* pattern, int pattern_len, int negate, uint32_t* bits, int mode,
                                uint32_t* scratch, void* stream) {
  clear_error();
  MQ_CHECK_ARG(n >= 0 && text_bytes >= 0, "negative size (n %lld, text_bytes %lld)", (long long)n,
               (long long)text_bytes);
  MQ_CHECK_ARG(pattern_len >= 1 && pattern_len <= MQ_CONTAINS_MAX_BYTES, "pattern_len must be in [1, %d] (got %d)",
               MQ_CONTAINS_MAX_BYTES, pattern_len);
  MQ_CHECK_ARG(pattern, "NULL pattern");
  MQ_CHECK_ARG(mode == MQ_MASK_SET || mode == MQ_MASK_AND || mode == MQ_MASK_OR, "bad mask mode %d", mode);
  MQ_CHECK_ARG(negate == 0 || negate == 1, "negate must be 0 or 1 (got %d)", negate);
  if (n == 0) return MQ_OK;
  MQ_CHECK_ARG(offsets && bits && scratch && (text || text_bytes == 0), "NULL buffer");
  MQ_CHECK_ARG(bits != scratch, "scratch must not be bits");
  MQ_CHECK_ARG((reinterpret_cast<uintptr_t>(text) & 15) == 0, "text must be 16-byte aligned");
  const int64_t spans = (text_bytes + kSpan - 1) / kSpan;
  MQ_CHECK_ARG(spans <= 0x7fffffff, "text_bytes %lld out of range", (long long)text_bytes);
  const int dev = pointer_device(bits);
  MQ_CHECK_ARG(dev >= 0 && pointer_device(offsets) == dev && pointer_device(scratch) == dev &&
                   (text_bytes == 0 || pointer_device(text) == dev),
               "text, offsets, bits and scratch must be device memory of one GPU");
  DeviceGuard dg(dev);  // the launches run on the buffers' GPU (stream: that device's)
  hipStream_t s = (hipStream_t)stream;
  const int64_t words = (n + 31) / 32;
  MQ_HIP(hipMemsetAsync(scratch, 0, (size_t)words * 4, s));
  if (spans > 0) {
    PatWords pw{};
    memcpy(pw.w, pattern, (size_t)pattern_len);
    hipLaunchKernelGGL(contains_scan_kernel, dim3((unsigned)spans), dim3(kThreads), 0, s,
                       (const unsigned char*)text, text_bytes, offsets, n, pw, pattern_len, (unsigned*)scratch);
    MQ_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(contains_finish_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s,
                     (const unsigned*)scratch, n, negate, (unsigned*)bits, mode);
  MQ_HIP(hipGetLastError());
  return MQ_OK;
}
