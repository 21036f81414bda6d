// retrieval.hip -- full-corpus text-to-video retrieval evaluation (eval_retrieval.py:100-115, eval_retrieval_tsv.py:53-91) on gfx950:
// the clip mean of the video bank, the assembly of a block of (text, video) fusion sequences straight from the two banks (row indices
// computed here: the pair loop uploads nothing per block), and the sigmoid + ground-truth rank of every text row of the score matrix.
#include "common.h"

namespace {

inline int nblk(long n, int per) { return (int)((n + per - 1) / per); }

// dst[b][r][:] = bf16( (1/clips) * sum_c src[b][c][r][:] ), f32 sums; one thread per 8 channels of one output row
__global__ void clip_mean_kernel(const u16* __restrict__ src, u16* __restrict__ dst, int B, int clips, int rows, int H) {
  const int nch = H / 8;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)B * rows * nch) return;
  const int ch = (int)(i % nch);
  const long br = i / nch;                                 // b * rows + r
  const long b = br / rows, r = br - b * rows;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < clips; ++c) {
    float f[8];
    unpack_bf8(*reinterpret_cast<const uint4*>(src + ((b * clips + c) * rows + r) * H + ch * 8), f);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += f[k];
  }
  const float inv = 1.0f / (float)clips;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] *= inv;
  *reinterpret_cast<uint4*>(dst + br * H + ch * 8) = pack_bf8(acc);
}

// pair p = t * nv + v of the block (texts t0 + t, videos v0 + v): rows [0, Lv) of sequence p = video bank rows of video v0 + v, rows
// [Lv, Lv + X) = text bank rows of text t0 + t; key mask = 1 over the video part, then the text's mask.  One thread per 16 bytes of a row.
__global__ void pair_assemble_kernel(const u16* __restrict__ vid, const u16* __restrict__ txt, const uint8_t* __restrict__ txt_mask,
                                     u16* __restrict__ seq, uint8_t* __restrict__ keymask, int Lv, int X, int H, int t0, int v0, int nv, long P) {
  const int nch = H / 8, Lq = Lv + X;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= P * Lq * nch) return;
  const int ch = (int)(i % nch);
  const long row = i / nch;                                // p * Lq + r
  const long p = row / Lq;
  const int r = (int)(row - p * Lq);
  const long t = t0 + p / nv, v = v0 + p % nv;
  const u16* s = r < Lv ? vid + (v * Lv + r) * H : txt + (t * X + (r - Lv)) * H;
  *reinterpret_cast<uint4*>(seq + row * H + ch * 8) = *reinterpret_cast<const uint4*>(s + ch * 8);
  if (ch == 0) keymask[row] = r < Lv ? (uint8_t)1 : (uint8_t)(txt_mask[t * X + (r - Lv)] != 0);
}

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

// one workgroup per text row: scores = sigmoid(logits) in place; rank = 1 + #{v : s_v > s_gt} + #{v < gt : s_v == s_gt} -- the
// 1-based position of the ground-truth video after a stable sort by descending score (ties keep bank order).  gt out of [0, Nv): -1.
__global__ void __launch_bounds__(256) rank_kernel(float* __restrict__ s, int Nv, long ld, const int32_t* __restrict__ gt, int32_t* __restrict__ rank) {
  __shared__ int cnt;
  const long row = blockIdx.x;
  float* r = s + row * ld;
  const int g = gt[row];
  const bool ok = g >= 0 && g < Nv;
  const float sg = ok ? sigmoid_f32(r[g]) : 0.f;          // read before any thread overwrites the row
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  int c = 0;
  for (int v = threadIdx.x; v < Nv; v += blockDim.x) {
    const float x = sigmoid_f32(r[v]);
    r[v] = x;
    c += (x > sg) || (x == sg && v < g);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(&cnt, c);
  __syncthreads();
  if (threadIdx.x == 0) rank[row] = ok ? cnt + 1 : -1;
}

}  // namespace

#define ST reinterpret_cast<hipStream_t>(stream)

extern "C" int vmvm_clip_mean_bf16(const void* src, void* dst, int32_t B, int32_t clips, int32_t rows, int32_t H, void* stream) {
  if (!src || !dst || B <= 0 || clips <= 0 || rows <= 0 || H <= 0 || (H & 7)) return VMVM_EINVAL;
  if ((reinterpret_cast<uintptr_t>(src) & 15) || (reinterpret_cast<uintptr_t>(dst) & 15)) return VMVM_EINVAL;
  if ((int64_t)B * clips * rows * H >= ((int64_t)1 << 40)) return VMVM_ENOSUPPORT;
  hipLaunchKernelGGL(clip_mean_kernel, dim3(nblk((long)B * rows * (H / 8), 256)), dim3(256), 0, ST, reinterpret_cast<const u16*>(src),
                     reinterpret_cast<u16*>(dst), B, clips, rows, H);
  VMVM_CHECK_LAUNCH();
  return VMVM_OK;
}

extern "C" int vmvm_retrieval_assemble(const void* vid_bank, int32_t Nv, int32_t Lv, const void* txt_bank, const uint8_t* txt_mask, int32_t Nt,
                                       int32_t X, int32_t H, int32_t t0, int32_t nt, int32_t v0, int32_t nv, void* seq, uint8_t* keymask,
                                       void* stream) {
  if (!vid_bank || !txt_bank || !txt_mask || !seq || !keymask) return VMVM_EINVAL;
  if (Nv <= 0 || Nt <= 0 || Lv <= 0 || X <= 0 || H <= 0 || (H & 7) || nt <= 0 || nv <= 0 || t0 < 0 || v0 < 0) return VMVM_EINVAL;
  if ((int64_t)t0 + nt > Nt || (int64_t)v0 + nv > Nv) return VMVM_EINVAL;               // the block lies inside both banks
  if ((reinterpret_cast<uintptr_t>(vid_bank) & 15) || (reinterpret_cast<uintptr_t>(txt_bank) & 15) || (reinterpret_cast<uintptr_t>(seq) & 15)) return VMVM_EINVAL;
  const int64_t P = (int64_t)nt * nv;
  if (P * (Lv + X) * (H / 8) >= ((int64_t)1 << 40)) return VMVM_ENOSUPPORT;
  hipLaunchKernelGGL(pair_assemble_kernel, dim3(nblk((long)P * (Lv + X) * (H / 8), 256)), dim3(256), 0, ST, reinterpret_cast<const u16*>(vid_bank),
                     reinterpret_cast<const u16*>(txt_bank), txt_mask, reinterpret_cast<u16*>(seq), keymask, Lv, X, H, t0, v0, nv, (long)P);
  VMVM_CHECK_LAUNCH();
  return VMVM_OK;
}

extern "C" int vmvm_retrieval_rank(float* scores, int32_t Nt, int32_t Nv, int32_t ld, const int32_t* gt, int32_t* rank, void* stream) {
  if (!scores || !gt || !rank || Nt <= 0 || Nv <= 0 || ld < Nv) return VMVM_EINVAL;
  hipLaunchKernelGGL(rank_kernel, dim3(Nt), dim3(256), 0, ST, scores, Nv, (long)ld, gt, rank);
  VMVM_CHECK_LAUNCH();
  return VMVM_OK;
}
