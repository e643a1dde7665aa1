// pm_graph_u8.hip — the exact kNN over uint8 rows on the int8 matrix cores
// (pm_knn_u8, pm_build_graph_u8).  For rows of values 0..255
// and dim <= 256 every squared distance is an integer below 2^24, so the
// integer distance converted to float is the reference's L2Dist bit for bit:
// no re-rank, no certificate, no fallback.
//
//   k_u8_bias     rows to the signed operand: x' = x - 128 (x ^ 0x80 as int8),
//                 padded with 0 to dp (the next multiple of 64), and the row's
//                 constant c = sum x'^2 over the dim real coordinates
//   k_knn_i8      per query row the 128 smallest (distance, id) keys over all
//                 base rows, dist = c(q) + c(x) - 2 q'.x' with q'.x' from
//                 mfma_i32_32x32x32_i8, and the first K of them written out
//   k_u8_to_f32   the rows as f32, for the build's robustPrune stages
//
// The tile walk is k_knn_bf16x3<DP, 128>'s (pm_graph.hip) with one operand tile;
// the lists, the tile epilogue and the emit are pm_graph_dev.h's.
#include <hip/hip_runtime.h>

#include "pm_internal.h"
#include "pm_graph_dev.h"

namespace pm {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int kU8Cols = 64;        // base rows per tile
constexpr int kU8Threads = 256;    // 4 waves: 2 row blocks x 2 column blocks of 32x32
constexpr int kU8MaxDim = 256;     // 256 * 255^2 < 2^24: every distance exact in f32
constexpr int kU8Pad = 16;         // bytes after a tile row in LDS

// One wave per row, four bytes per lane (dp <= 256 = 64 lanes x 4).  c is the
// constant of §10.4: sum (x - 128)^2 = |x|^2 - 256 sum x + 128^2 dim, at most
// 256 * 128^2 = 2^22.
__global__ void __launch_bounds__(kBlock) k_u8_bias(const uint8_t* __restrict__ rows, uint64_t n, uint32_t dim,
                                                    uint32_t dp, uint8_t* __restrict__ out,
                                                    int32_t* __restrict__ cst) {
  constexpr uint32_t W = kBlock / 64;
  const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (uint64_t r = (uint64_t)blockIdx.x * W + w; r < n; r += (uint64_t)gridDim.x * W) {
    const uint8_t* in = rows + r * dim;
    uint32_t word = 0;
    int32_t s = 0;
    #pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
      const uint32_t i = 4 * lane + j;
      if (i < dim) {
        const uint32_t v = in[i];
        const int32_t x = (int32_t)v - 128;
        s += x * x;
        word |= (v ^ 0x80u) << (8 * j);
      }
    }
    if (4 * lane < dp) *(uint32_t*)(out + r * dp + 4 * lane) = word;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (lane == 0) cst[r] = s;
  }
}

__global__ void __launch_bounds__(kBlock) k_u8_to_f32(const uint8_t* __restrict__ rows, uint64_t count,
                                                      float* __restrict__ out) {
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < count; i += (uint64_t)gridDim.x * kBlock)
    out[i] = (float)rows[i];
}

template <int DP>
struct KnnU8Lds : KnnLists<kKnnTop2, kU8Cols> {
  int8_t b[kU8Cols][DP + kU8Pad];           // padded rows: conflict-free 16-B fragment reads
};
static_assert(sizeof(KnnU8Lds<64>) == 103688 && sizeof(KnnU8Lds<256>) == 115976, "LDS budget of DESIGN.md §10.4");
static_assert(sizeof(KnnU8Lds<kU8MaxDim>) <= 160 * 1024, "LDS of one CU");

// A sorted key's integer distance as the float the caller reads (exact: < 2^24).
__device__ __forceinline__ uint64_t u8_key_f32(uint64_t x) {
  if (x == kNoKey) return x;
  return ((uint64_t)__float_as_uint((float)(uint32_t)(x >> 32)) << 32) | (uint32_t)x;
}

// Per query row the 128 smallest ((uint32) dist << 32 | id) keys over the N base
// rows, and of those the first K (self dropped when self_base) to out [M][K],
// their distances as floats to dist_out when given, their number to len [M].
// X, Q: biased rows of DP bytes (k_u8_bias), xc, qc their constants.  A lane's
// A and B fragments of k-step s are bytes [32 s + 16 h, + 16) of its row: the
// same k for both operands, which is all the sum over k needs.
template <int DP>
__global__ void __launch_bounds__(kU8Threads) k_knn_i8(const int8_t* __restrict__ X, const int32_t* __restrict__ xc,
                                                       uint64_t N, const int8_t* __restrict__ Q,
                                                       const int32_t* __restrict__ qc, uint64_t M, uint32_t K,
                                                       int self_base, uint32_t* __restrict__ out,
                                                       float* __restrict__ dist_out, uint32_t* __restrict__ len) {
  constexpr int KS = DP / 32;
  constexpr int CH = kU8Cols * DP / 16;             // 16-B chunks per tile
  constexpr int PER = CH / kU8Threads;
  constexpr int MR = kKnnRows / (kU8Threads / 64);  // rows each wave merges
  static_assert(DP % 64 == 0 && CH % kU8Threads == 0, "tile chunks");
  __shared__ KnnU8Lds<DP> L;
  const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const uint32_t rb = 32 * (w & 1), cb = 32 * (w >> 1);
  const uint32_t r32 = lane & 31, h = lane >> 5;
  const uint64_t row0 = (uint64_t)blockIdx.x * kKnnRows;
  knn_lists_init<kU8Threads>(L, tid);

  i32x4 a[KS];
  {
    const uint64_t qr = row0 + rb + r32;
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (qr < M) a[s] = *(const i32x4*)(Q + qr * DP + 32 * s + 16 * h);
      else a[s] = i32x4{0, 0, 0, 0};
    }
  }
  int32_t qcr[16];
  uint32_t thi[16];
  knn_rows_init(qc, row0, M, rb, h, qcr, thi);
  const uint64_t T = (N + kU8Cols - 1) / kU8Cols;
  uint4 pre[PER];
  auto load_tile = [&](uint64_t t) {
    const uint64_t c0 = t * kU8Cols;
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kU8Threads;
      const uint32_t j = q / (DP / 16), off = (q % (DP / 16)) * 16;
      pre[p] = c0 + j < N ? *(const uint4*)(X + (c0 + j) * DP + off) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_tile = [&]() {
    #pragma unroll
    for (int p = 0; p < PER; ++p) {
      const uint32_t q = tid + p * kU8Threads;
      const uint32_t j = q / (DP / 16), off = (q % (DP / 16)) * 16;
      *(uint4*)&L.b[j][off] = pre[p];
    }
  };
  load_tile(0);
  store_tile();
  __syncthreads();
  uint32_t par = 0;   // t & 1, carried by knn_tile_end
  for (uint64_t t = 0; t < T; ++t) {
    if (t + 1 < T) load_tile(t + 1);   // in flight during the MFMAs
    i32x16 acc = {};
    #pragma unroll
    for (int s = 0; s < KS; ++s) {
      const i32x4 b = *(const i32x4*)&L.b[cb + r32][32 * s + 16 * h];
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[s], b, acc, 0, 0, 0);
    }
    const uint64_t col = t * kU8Cols + cb + r32;
    knn_tile_end<kU8Threads>(
        L, par, col, N, xc, rb, h, thi, [=](int i, int32_t cn) { return (uint32_t)(qcr[i] + cn - 2 * acc[i]); },
        [&] { if (t + 1 < T) store_tile(); });
  }
  for (uint32_t r = w * MR; r < w * MR + MR; ++r) {
    const uint64_t qr = row0 + r;
    if (qr < M) {   // uniform per wave
      TopKeys<kKnnTop2> t = TopKeys<kKnnTop2>::load(L.top[r], lane);
      #pragma unroll
      for (int i = 0; i < t.H; ++i) t.v[i] = u8_key_f32(t.v[i]);
      t.emit(qr, K, self_base, lane, out, dist_out, len);
    }
  }
}

}  // namespace pm

namespace pmk {
uint32_t knn_u8_max_dim() { return kU8MaxDim; }
uint32_t knn_u8_pad_dim(uint32_t dim) { return dim == 0 || dim > (uint32_t)kU8MaxDim ? 0 : (dim + 63) / 64 * 64; }

void u8_bias(hipStream_t st, const uint8_t* rows, uint64_t n, uint32_t dim, uint32_t dp, void* out, int32_t* cst) {
  if (!n) return;
  hipLaunchKernelGGL(k_u8_bias, dim3(gclamp(gcdiv(n, kBlock / 64))), dim3(kBlock), 0, st, rows, n, dim, dp,
                     (uint8_t*)out, cst);
}
void u8_to_f32(hipStream_t st, const uint8_t* rows, uint64_t count, float* out) {
  if (!count) return;
  hipLaunchKernelGGL(k_u8_to_f32, dim3(gclamp((count + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, rows, count, out);
}
// dp: 64, 128, 192 or 256 (knn_u8_pad_dim); K in [1, 128]
void knn_i8(hipStream_t st, const void* X, const int32_t* xc, uint64_t N, const void* Q, const int32_t* qc, uint64_t M,
            uint32_t dp, uint32_t K, bool self_base, uint32_t* out, float* dist, uint32_t* len) {
  if (!M) return;
  const dim3 grid(gcdiv(M, kKnnRows)), block(kU8Threads);
  const int8_t *x = (const int8_t*)X, *q = (const int8_t*)Q;
  switch (dp) {
    case 64: hipLaunchKernelGGL(k_knn_i8<64>, grid, block, 0, st, x, xc, N, q, qc, M, K, (int)self_base, out, dist, len); break;
    case 128: hipLaunchKernelGGL(k_knn_i8<128>, grid, block, 0, st, x, xc, N, q, qc, M, K, (int)self_base, out, dist, len); break;
    case 192: hipLaunchKernelGGL(k_knn_i8<192>, grid, block, 0, st, x, xc, N, q, qc, M, K, (int)self_base, out, dist, len); break;
    default: hipLaunchKernelGGL(k_knn_i8<256>, grid, block, 0, st, x, xc, N, q, qc, M, K, (int)self_base, out, dist, len); break;
  }
}
}  // namespace pmk
