// qamc.hip -- video token selection of the fc-head multiple-choice QA model (VIOLET_QAMC.select_vid_token, main_qamc.py:55-83) on gfx950.
// Per clip b and selection head h (n heads of width d = H / n): s = q_h k_h^T / sqrt(H) + key mask, c = softmax over the keys summed over
// the queries, dropout on c, then the straight-through gumbel_softmax(hard=True), whose forward value is the one-hot of
// argmax_k(c_k + g_k) (tau only rescales before the arg-max).  The clip keeps the union of its heads' arg-maxes, ANDed with its mask.
//
// One workgroup per (clip, head): q_h / k_h of the clip staged in LDS (bf16, exact copies of the GEMM outputs).  Pass 1: one thread per
// query row, running max / sum over the keys in key order.  Pass 2: one thread per key, the column sum over the queries in query order.
// The arg-max reduction is exact (lowest index wins ties), so the result is bit-reproducible and independent of the other clips.
#include "common.h"

namespace {

inline int nblk(long n, int per) { return (int)((n + per - 1) / per); }

constexpr int SEL_THREADS = 256;

// (v, j) beats (v2, j2): larger value, lower index on a tie
__device__ __forceinline__ bool sel_better(float v, int j, float v2, int j2) { return v > v2 || (v == v2 && j < j2); }

template <int D>
__device__ __forceinline__ void load_row(const u16* __restrict__ src, float (&f)[D]) {
#pragma unroll
  for (int e = 0; e < D; ++e) f[e] = bf2f(src[e]);
}

template <int D>
__global__ __launch_bounds__(SEL_THREADS) void token_select_kernel(const u16* __restrict__ q, const u16* __restrict__ k, const uint8_t* __restrict__ vmask,
                                                                   const float* __restrict__ noise, int Lv, int H, int n, float scale,
                                                                   float dropout_p, uint64_t seed_d, uint64_t off_d, uint64_t seed_n, uint64_t off_n,
                                                                   int32_t* __restrict__ idx) {
  extern __shared__ float smf[];                         // [Lv] row max, [Lv] 1 / row sum, then bf16 [Lv][D] q and [Lv][D] k
  float* mrow = smf;
  float* irow = smf + Lv;
  u16* qs = reinterpret_cast<u16*>(smf + 2 * Lv);
  u16* ks = qs + (size_t)Lv * D;
  __shared__ float red_v[SEL_THREADS / 64];
  __shared__ int red_j[SEL_THREADS / 64];
  const int b = blockIdx.x / n, h = blockIdx.x - b * n, tid = threadIdx.x;
  const uint8_t* mk = vmask ? vmask + (size_t)b * Lv : nullptr;
  for (int e = tid; e < Lv * D; e += SEL_THREADS) {
    const int r = e / D, c = e - r * D;
    const size_t g = ((size_t)b * Lv + r) * H + (size_t)h * D + c;
    qs[e] = q[g];
    ks[e] = k[g];
  }
  __syncthreads();
  int live = 0;
  for (int j = tid; j < Lv; j += SEL_THREADS) live |= (!mk || mk[j] != 0);
  // every key masked: the reference's additive mask moves every score onto finfo.min, i.e. a uniform softmax over all keys
  const bool all_masked = __syncthreads_or(live) == 0;
  // pass 1: query row i -> max and 1 / sum of its scores over the live keys, keys in order
  for (int i = tid; i < Lv; i += SEL_THREADS) {
    float qi[D];
    load_row<D>(qs + (size_t)i * D, qi);
    float m = -__builtin_inff(), l = 0.f;
    for (int j = 0; j < Lv; ++j) {
      if (mk && !all_masked && mk[j] == 0) continue;
      float kj[D];
      load_row<D>(ks + (size_t)j * D, kj);
      float a = 0.f;
#pragma unroll
      for (int e = 0; e < D; ++e) a = fmaf(qi[e], kj[e], a);
      const float s = all_masked ? 0.f : a * scale;
      if (s > m) { l = l * expf(m - s) + 1.f; m = s; }
      else l += expf(s - m);
    }
    mrow[i] = m;
    irow[i] = 1.f / l;
  }
  __syncthreads();
  // pass 2: key j -> c_j = sum_i p_ij, queries in order; dropout; + gumbel noise; running arg-max of this thread's keys
  const bool has_drop = dropout_p > 0.f;
  const uint32_t thr = dropout_threshold(dropout_p);
  const float keep = has_drop ? 1.0f / (1.0f - dropout_p) : 1.0f;
  float best = -__builtin_inff();
  int bj = 0x7fffffff;
  for (int j = tid; j < Lv; j += SEL_THREADS) {
    float c = 0.f;
    if (all_masked || !mk || mk[j] != 0) {
      float kj[D];
      load_row<D>(ks + (size_t)j * D, kj);
      for (int i = 0; i < Lv; ++i) {
        float qi[D];
        load_row<D>(qs + (size_t)i * D, qi);
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < D; ++e) a = fmaf(qi[e], kj[e], a);
        const float s = all_masked ? 0.f : a * scale;
        c = fmaf(expf(s - mrow[i]), irow[i], c);
      }
    }
    const uint64_t el = ((uint64_t)b * n + h) * (uint64_t)Lv + j;
    if (has_drop) {
      uint32_t bits[8];
      dropout_bits8(seed_d, off_d, el >> 3, bits);
      c = bits[el & 7] < thr ? 0.f : c * keep;
    }
    float g;
    if (noise) {
      g = noise[el];
    } else {                                             // g = -log(E), E = -log(U) ~ Exp(1), U in (0, 1] (24 bits)
      const uint64_t ctr = off_n + (el >> 2);
      const uint4 r = philox4x32_7(make_uint4((uint32_t)ctr, (uint32_t)(ctr >> 32), 0x9a7bu, 0u), make_uint2((uint32_t)seed_n, (uint32_t)(seed_n >> 32)));
      const uint32_t w = (el & 3) == 0 ? r.x : (el & 3) == 1 ? r.y : (el & 3) == 2 ? r.z : r.w;
      const float u = (float)((w >> 8) + 1u) * (1.0f / 16777216.0f);
      g = -logf(-logf(u));
    }
    const float v = c + g;
    if (sel_better(v, j, best, bj)) { best = v; bj = j; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(best, o, 64);
    const int j2 = __shfl_xor(bj, o, 64);
    if (sel_better(v2, j2, best, bj)) { best = v2; bj = j2; }
  }
  if ((tid & 63) == 0) { red_v[tid >> 6] = best; red_j[tid >> 6] = bj; }
  __syncthreads();
  if (tid == 0) {
    float bv = red_v[0];
    int bjj = red_j[0];
#pragma unroll
    for (int w = 1; w < SEL_THREADS / 64; ++w)
      if (sel_better(red_v[w], red_j[w], bv, bjj)) { bv = red_v[w]; bjj = red_j[w]; }
    idx[(size_t)b * n + h] = bjj < Lv ? bjj : 0;         // (NaN scores everywhere: key 0, as torch's arg-max of an all-NaN row is not defined either)
  }
}

// sel[b][j] = mask[b][j] AND (some head of clip b selected key j); one thread per (clip, key), heads in order
__global__ void token_union_kernel(const int32_t* __restrict__ idx, const uint8_t* __restrict__ vmask, uint8_t* __restrict__ sel, int B, int Lv, int n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * Lv) return;
  const int b = (int)(i / Lv), j = (int)(i - (long)b * Lv);
  uint8_t hit = 0;
  for (int h = 0; h < n; ++h) hit |= (uint8_t)(idx[(size_t)b * n + h] == j);
  sel[i] = (uint8_t)(hit && (!vmask || vmask[i] != 0));
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int vmvm_video_token_select(const void* q, const void* k, const uint8_t* vis_mask, const float* noise, int32_t B, int32_t Lv, int32_t H,
                                       int32_t n, float dropout_p, uint64_t seed_drop, uint64_t off_drop, uint64_t seed_noise, uint64_t off_noise,
                                       int32_t* idx, uint8_t* sel, void* stream) {
  if (!q || !k || !idx || !sel) return VMVM_EINVAL;
  if (B <= 0 || Lv <= 0 || H <= 0 || n <= 0 || H % n != 0) return VMVM_EINVAL;
  const int d = H / n;
  if (d != 4 && d != 8 && d != 16) return VMVM_EINVAL;
  if (Lv > VMVM_VIDEO_TOKEN_SELECT_MAX_LV) return VMVM_EINVAL;
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return VMVM_EINVAL;                       // (NaN fails too)
  if ((reinterpret_cast<uintptr_t>(q) & 1) || (reinterpret_cast<uintptr_t>(k) & 1)) return VMVM_EINVAL;
  if ((int64_t)B * n >= ((int64_t)1 << 31) || (int64_t)B * Lv * H >= ((int64_t)1 << 40)) return VMVM_ENOSUPPORT;
  const size_t lds = (size_t)Lv * (2 * sizeof(float) + 2 * (size_t)d * sizeof(u16));
  const float scale = 1.0f / sqrtf((float)H);
  const u16* qq = reinterpret_cast<const u16*>(q);
  const u16* kk = reinterpret_cast<const u16*>(k);
  if (d == 4)
    hipLaunchKernelGGL(token_select_kernel<4>, dim3(B * n), dim3(SEL_THREADS), lds, ST, qq, kk, vis_mask, noise, Lv, H, n, scale, dropout_p,
                       seed_drop, off_drop, seed_noise, off_noise, idx);
  else if (d == 8)
    hipLaunchKernelGGL(token_select_kernel<8>, dim3(B * n), dim3(SEL_THREADS), lds, ST, qq, kk, vis_mask, noise, Lv, H, n, scale, dropout_p,
                       seed_drop, off_drop, seed_noise, off_noise, idx);
  else
    hipLaunchKernelGGL(token_select_kernel<16>, dim3(B * n), dim3(SEL_THREADS), lds, ST, qq, kk, vis_mask, noise, Lv, H, n, scale, dropout_p,
                       seed_drop, off_drop, seed_noise, off_noise, idx);
  VMVM_CHECK_LAUNCH();
  hipLaunchKernelGGL(token_union_kernel, dim3(nblk((long)B * Lv, 256)), dim3(256), 0, ST, idx, vis_mask, sel, B, Lv, n);
  VMVM_CHECK_LAUNCH();
  return VMVM_OK;
}
