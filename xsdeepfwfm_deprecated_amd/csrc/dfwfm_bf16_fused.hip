// dfwfm_bf16_fused.hip -- the forward with a bf16 deep tower in ONE launch (include/dfwfm_bf16_fused.h).
//
// The per-layer path (dfwfm_bf16.hip) is the gather launch, a launch per hidden layer and a combine launch, with the
// f32 E rows, every bf16 activation and the last layer's shares in the caller's workspace.  Here one workgroup of
// eight waves owns ROWS = 16 RT rows of one batch (RT = 1, 2, 4) and carries them from Xi / Xv to the logits:
//
//   stage 1  descriptors, keys, the gather of the f32 E tile into LDS, the table / fwlw first order and the FwFM /
//            FM second order as U'E pieces -- the arithmetic of the gather launch (fwd_kernel PART 3 with
//            kP3Pieces), per 16-row sub-tile, so first + second are the bits dfwfm_forward_gather writes.  The
//            gather and the first + second reduction are the stage_* functions of dfwfm_fused_stage.h, which the
//            int8 forward (dfwfm_int8.hip) calls too; the staging and the shallow half stand in both kernel bodies
//            (that header says why);
//   stage 2  the hidden layers on v_mfma_f32_16x16x32_bf16: the weights are the A operand, 16-byte fragments of the
//            pack of dfwfm_model_pack_bf16 streamed from L2 (wave w owns output tiles w, w + 8, ... for every row
//            sub-tile, so a fragment feeds RT MFMAs), the activations the B operand, read from the LDS tile: layer 1
//            from the f32 E tile, rounded with v_cvt_pk_bf16_f32 on the way, later layers from the bf16 tile the
//            layer before wrote IN PLACE of it (a barrier between a layer's K loop and its epilogue: every wave
//            holds all its accumulators in registers before any writes);
//   stage 3  the last layer's share of deep per 16-neuron tile, as layer_epilogue forms it, into LDS [row][NT];
//   stage 4  the shares added in tile order, logit = (first_second + deep) + bias, as bf16_combine_kernel.
//
// Every sum has the order the contract of include/dfwfm_bf16.h fixes (one accumulator per output element, K steps
// c = 0 .. KC - 1 in turn), so the logits are the per-layer path's bit for bit, whatever RT.
//
// LDS (floats): [tile: ROWS x SE f32, then ROWS x SB bf16 in place][fs: ROWS][scratch: descriptors, lw, fwlw, first
// order, FwFM column sums -- dead after stage 1, then the last layer's shares [ROWS][NT]].  SE = 4 mod 8 floats and
// SB = 8 mod 16 bf16: the 16 rows a quarter wave reads 16 bytes of start 16 bytes apart modulo 256, no bank conflict.
// Rows past the batch hold zeros and run through every stage (every wave reaches every barrier); nothing of them is
// written out.
//
// The folded layer 1 (include/dfwfm_bf16_fold.h, the FOLD forms): a tile row is [xsh floats unused][E: F D][Xv: num]
// [zeros], xsh = (-num D) mod 4, so that the categorical block at column num D starts 16-byte aligned; the gather's
// numerical rows also store their Xv behind column F D, and layer 1 reads its K steps from column num D on against the
// fragments of bf16_fold_pack_kernel (categorical columns of bf16(W1) | bf16(P) | zeros).  xsh + WE is a multiple of 8,
// so SE = 4 mod 8 still.  The FwFM then clamps its padded fields to F (Xv lies where field F would).  Layers 2..H, the
// shallow half and the unfolded forms are untouched.
//
// The workgroup shape (kF*), the stage-1 scratch, the weight fragment ring of the K loop, the last layer's share, the
// logits and the launch are dfwfm_fused_stage.h's too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_device.h"
#include "dfwfm_fused_stage.h"
#include "dfwfm_internal.h"

namespace dfwfm {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// two f32 to two bf16, round to nearest even, NaN kept: lo in bits 0-15
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

struct FusedLds {
  int tile, fs, part, total;
  StageLds st;
};

__host__ __device__ inline FusedLds fused_layout(int rows, int F, int D, int NT, int SE, int SB) {
  FusedLds L;
  int o = 0;
  const int tf = rows * SE, tb = rows * SB / 2;
  L.tile = o;  o += r4(tf > tb ? tf : tb);
  L.fs = o;    o += rows;
  L.st = stage_layout(o, rows, F, D);
  const int s = L.st.end;
  int t = o;
  L.part = t;  t += rows * NT;
  L.total = r4(s > t ? s : t);
  return L;
}

// the B fragment of K step c of one 16-row sub-tile, as the bf16x8 the MFMA takes: from the f32 E tile (two 16-byte
// reads, rounded: ActFrag<true> of the per-layer path) or from the bf16 tile (one 16-byte read)
template <bool F32IN>
__device__ __forceinline__ u32x4 act_frag(const char* p) {
  if constexpr (F32IN) {
    const f32x4 lo = reinterpret_cast<const f32x4*>(p)[0];
    const f32x4 hi = reinterpret_cast<const f32x4*>(p)[1];
    return u32x4{cvt_pk_bf16(lo[0], lo[1]), cvt_pk_bf16(lo[2], lo[3]), cvt_pk_bf16(hi[0], hi[1]),
                 cvt_pk_bf16(hi[2], hi[3])};
  } else {
    return *reinterpret_cast<const u32x4*>(p);
  }
}

// one layer's K loop of one wave: its kFTPW output tiles (wt[j]: the tile's fragments of K step 0) times the RT row
// sub-tiles (brow: this lane's 16 bytes of K step 0 in sub-tile 0; rt_bytes / c_bytes to the next sub-tile / K step).
// The weight fragment sets go through the ring of ring_k_loop.  The activation fragments come from LDS in their own
// step: the other waves of the SIMD cover that latency, and a ring of them cost the 32-row form its second workgroup
// per CU (registers).
template <int RT, bool F32IN>
__device__ __forceinline__ void fused_k_loop(f32x4 (&acc)[RT][kFTPW], const u32x4* const (&wt)[kFTPW], int lane,
                                             const char* brow, int rt_bytes, int KC) {
  constexpr int c_bytes = F32IN ? 128 : 64;
  ring_k_loop<ring_depth(RT), kFTPW>(wt, lane, KC, [&](int c, const u32x4(&wq)[kFTPW]) {
    u32x4 aq[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) aq[i] = act_frag<F32IN>(brow + i * rt_bytes + c * c_bytes);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const bf16x8 x = __builtin_bit_cast(bf16x8, aq[i]);
#pragma unroll
      for (int j = 0; j < kFTPW; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq[j]), x, acc[i][j], 0, 0, 0);
    }
  });
}

// RT: 16-row sub-tiles per workgroup; QR: some field may be a QR embedding (false: the gather carries no second
// operand); FOLD: layer 1 folded (include/dfwfm_bf16_fold.h) -- a form of its own, so that the unfolded one keeps its
// code (and registers) exactly
template <int RT, bool QR, bool FOLD>
__global__ void __launch_bounds__(kFTH) __attribute__((amdgpu_waves_per_eu(RT == 4 ? 2 : 4)))
bf16_fused_kernel(const FwdArgs p, const Bf16FusedGeo q) {
  constexpr int D = 10;
  constexpr int ROWS = 16 * RT;
  constexpr int LR = RT == 1 ? 4 : (RT == 2 ? 5 : 6);  // log2(ROWS)
  static_assert(RT == 1 || RT == 2 || RT == 4, "16, 32 or 64 rows");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = p.F;
  const int flags = p.flags;
  const int Fp = r4(F);
  const int SE = q.SE, SB = q.SB;
  const int xsh = FOLD ? q.xsh : 0, k0 = FOLD ? q.k0 : 0, nxv = FOLD ? q.nxv : 0;
  const FusedLds L = fused_layout(ROWS, F, D, p.NT, SE, SB);
  float* etile = smem + L.tile + xsh;  // (the folded layer 1: the categorical block 16-byte aligned)
  uint16_t* atile = reinterpret_cast<uint16_t*>(smem + L.tile);
  float* fs = smem + L.fs;
  const StageScratch sc = stage_scratch(smem, L.st);
  float* part = smem + L.part;
  const TileRef tr = tile_ref<ROWS>(p);  // batch set: this workgroup's batch

  // ---- stage 1: descriptors and shallow parameters to LDS, the E tile's zero padding; then dfwfm_fused_stage.h ------
  for (int i = tid; i < 7 * F; i += kFTH)
    reinterpret_cast<u32x2*>(sc.desc)[i] = reinterpret_cast<const u32x2*>(p.fields)[i];
  if (flags & kFoFwlw)
    for (int i = tid; i < F * D; i += kFTH) sc.fwlw[i] = p.fwlw[i];
  if ((flags & kFoLw) && tid < F) sc.lw[tid] = p.lw[tid];
  {
    // columns [F D, WE): layer 1 reads K steps of 32 up to k0 + KC0 * 32, the FwFM fields up to 4 S (the folded
    // layer 1's Xv columns are among them: the gather's numerical rows write them after the barrier)
    const int zc = F * D;
    const int w = q.WE - zc;
    for (int i = tid; i < ROWS * w; i += kFTH) {
      const int b = i / w;
      etile[b * SE + zc + (i - b * w)] = 0.f;
    }
  }
  __syncthreads();
  stage_gather<RT, QR, FOLD>(p, tr, sc, etile, SE, nxv, tid);
  __syncthreads();
  // ---- the shallow half: the expressions of fwd_kernel PART 3 (pieces form), per 16-row sub-tile ---------------------
  if (flags & kFoFwlw) {
    for (int r = tid; r < ROWS * F; r += kFTH) {
      const int f = r >> LR;
      const int b = r & (ROWS - 1);
      const float* e = etile + b * SE + f * D;
      const float* w = sc.fwlw + f * D;
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < D; ++d) s += e[d] * w[d];
      sc.fo[b * Fp + f] = s;
    }
  }
  if (flags & kHasSecond) {
    // Y = U' E (rows k: fields, MT tiles of 16; columns n = b D + d of a sub-tile's 16 samples: D tiles of 16;
    // contraction over l: S steps of 4, from step 4 m on), second[b] = sum_{k, d} E[b, k, d] Y[k, b D + d]
    constexpr int SMAX = 4 * kFMT;
    const int MT = p.MT, S = p.S;
    float uf[kFMT][SMAX];
    {
      const float* up = p.upack;
#pragma unroll
      for (int m = 0; m < kFMT; ++m)
#pragma unroll
        for (int s = 0; s < SMAX; ++s) uf[m][s] = (m < MT && s >= 4 * m && s < S) ? up[(m * S + s) * 64 + lane] : 0.f;
    }
    for (int it = wave; it < RT * D; it += kFW) {
      const int rt = it / D;
      const int nt = it - rt * D;
      const int n = nt * 16 + (lane & 15);
      const int b = n / D;
      const int d = n - b * D;
      const float* ecol = etile + (rt * 16 + b) * SE + d;  // E[b][l][d] = ecol[l * D]
      f32x4 acc[kFMT];
#pragma unroll
      for (int m = 0; m < kFMT; ++m) acc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s0 = 0; s0 < SMAX; s0 += 4) {
        float bv[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int s = s0 + u;
          const int l = 4 * s + (lane >> 4);  // (the columns of fields past F are zeros; folded, Xv lies there)
          bv[u] = (s < S && (!FOLD || l < F)) ? ecol[l * D] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
          for (int m = 0; m < kFMT; ++m)
            if (4 * m <= s0 + u && s0 + u < S && m < MT)
              acc[m] = __builtin_amdgcn_mfma_f32_16x16x4f32(uf[m][s0 + u], bv[u], acc[m], 0, 0, 0);
      }
      float colv = 0.f;
#pragma unroll
      for (int m = 0; m < kFMT; ++m) {
        if (m < MT) {  // wave-uniform: the gather launch's kernel has exactly MT row tiles
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = 16 * m + 4 * (lane >> 4) + r;
            colv = fmaf(k < F ? ecol[(k < F ? k : 0) * D] : 0.f, acc[m][r], colv);
          }
        }
      }
      colv += __shfl_xor(colv, 16);
      colv += __shfl_xor(colv, 32);
      if (lane < 16) sc.part2[rt * 16 * D + n] = colv;  // column n's sum over k (row tiles in order)
    }
  }
  __syncthreads();
  stage_fs<RT>(p, sc, fs, lane, wave);

  // ---- stages 2 and 3: the hidden layers; the tile is read by every wave's K loop, then overwritten in place ----------
  const int rl = lane & 15, kq = lane >> 4;
  const int NT = p.NT;
  const u32x4* wl = reinterpret_cast<const u32x4*>(q.w1);
  for (int h = 0; h < p.H; ++h) {
    const bool last = h == p.H - 1;
    const int KC = h == 0 ? q.KC0 : q.KCN;
    const u32x4* wt[kFTPW];
#pragma unroll
    for (int j = 0; j < kFTPW; ++j) {
      int t = wave + kFW * j;
      t = t < NT ? t : NT - 1;  // clamped duplicates, results discarded
      wt[j] = wl + (size_t)t * KC * 64;
    }
    f32x4 acc[RT][kFTPW];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < kFTPW; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (h == 0)
      fused_k_loop<RT, true>(acc, wt, lane, reinterpret_cast<const char*>(etile + rl * SE + k0 + 8 * kq), 16 * SE * 4,
                               KC);
    else
      fused_k_loop<RT, false>(acc, wt, lane, reinterpret_cast<const char*>(atile + rl * SB + 8 * kq), 16 * SB * 2, KC);
    __syncthreads();  // every wave has read the layer's input: the tile may be overwritten
    // the lane-derived epilogue values are recomputed per layer: hoisted out of the layer loop they stay live across
    // the K loops and spill
    int lv = lane;
    asm volatile("" : "+v"(lv));
    const int erl = lv & 15, ekq = lv >> 4;
    if (!last) {
      // the columns behind the last tile that the next layer's last K step reads (an odd tile count): zeros
      const int zw = q.KCN * 32 - NT * 16;  // 0 or 16
      for (int i = tid; i < ROWS * zw; i += kFTH) {
        const int b = i / zw;
        atile[b * SB + NT * 16 + (i - b * zw)] = 0;
      }
    }
#pragma unroll
    for (int j = 0; j < kFTPW; ++j) {
      const int t = wave + kFW * j;
      if (t >= NT) break;  // wave-uniform
      const int n0 = t * 16 + 4 * ekq;
      const f32x4 bq = *reinterpret_cast<const f32x4*>(p.mlp_b + (size_t)h * NT * 16 + n0);
      f32x4 fq = {0.f, 0.f, 0.f, 0.f};
      if (last) fq = *reinterpret_cast<const f32x4*>(p.fc + n0);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const int row = i * 16 + erl;
        f32x4 v;
#pragma unroll
        for (int r = 0; r < 4; ++r)  // padded neurons stay exactly 0
          v[r] = n0 + r < p.N ? relu_keep_nan(acc[i][j][r] + bq[r]) : 0.f;
        if (!last) {
          *reinterpret_cast<u32x2*>(atile + row * SB + n0) = u32x2{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3])};
        } else {  // uniform: every lane takes part in the shuffles
          last_layer_share(v, fq, lv, part + row * NT + t);
        }
      }
    }
    if (FOLD && h == 0)
      wl = reinterpret_cast<const u32x4*>(q.wn);  // layer 1's fragments were the folded ones, not the pack's
    else
      wl += (size_t)NT * KC * 64;
    __syncthreads();
  }

  // ---- stage 4: logit[b] = (first_second[b] + the shares in tile order) + bias -----------------------------------------
  stage_logits<ROWS>(p, tr, part, fs, NT, tid);
}

// dfwfm_model_fold_bf16: layer 1's fragments in the order of dfwfm_model_pack_bf16 over the folded K rows, one thread
// per (tile, K step, lane) and its 8 weights of neuron n = 16 t + (l & 15), rows k = 32 c + 8 (l >> 4) + j:
//   k < (F - num) D          bf16(W1[n][num D + k])                         (the categorical columns, field order)
//   k < (F - num) D + num    bf16(P[f][n]), P[f][n] = sum_d W1[n][f D + d] v_f[0][d], f = k - (F - num) D: the
//                            products are exact in f64, summed in f64 over d = 0..D-1 in that order, rounded to f32
//   else, and n >= N         0
__global__ void __launch_bounds__(256) bf16_fold_pack_kernel(const float* __restrict__ w1,
                                                             const FieldDev* __restrict__ fields,
                                                             u32x4* __restrict__ dst, int N, int F, int D, int num,
                                                             int KC, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63);
  const int64_t tc = i >> 6;
  const int c = (int)(tc % KC);
  const int n = (int)(tc / KC) * 16 + (lane & 15);
  const int k0 = c * 32 + 8 * (lane >> 4);
  const int K = F * D;
  const int KCat = (F - num) * D;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int k = k0 + j;
    v[j] = 0.f;
    if (n < N && k < KCat) {
      v[j] = w1[(size_t)n * K + num * D + k];
    } else if (n < N && k < KCat + num) {
      const int f = k - KCat;
      const float* w = w1 + (size_t)n * K + f * D;
      const float* e = fields[f].emb2;
      double acc = 0.0;
      for (int d = 0; d < D; ++d) acc += (double)w[d] * (double)e[d];
      v[j] = (float)acc;
    }
  }
  dst[i] = u32x4{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7])};
}

template <int RT>
hipError_t launch_rt(const FwdArgs& a, const Bf16FusedGeo& g, size_t lds, hipStream_t s) {
  auto k = g.nxv ? ((a.flags & kHasQR) ? bf16_fused_kernel<RT, true, true> : bf16_fused_kernel<RT, false, true>)
                 : ((a.flags & kHasQR) ? bf16_fused_kernel<RT, true, false> : bf16_fused_kernel<RT, false, false>);
  return launch_fused_kernel(k, a, g, 16 * RT, kFTH, lds, s);
}

inline int kc_of(int cols16) { return (cols16 * 16 + 31) / 32; }

// fold: the geometry of the folded layer 1 (include/dfwfm_bf16_fold.h); the pointers are the caller's to fill
Bf16FusedGeo fused_geo(int F, int num, int D, int NT, int NC0, int W0, bool fold) {
  Bf16FusedGeo g;
  g.w1 = g.wn = nullptr;
  g.KC0 = fold ? bf16_fold_steps(F, num, D) : kc_of(NC0);
  g.KCN = kc_of(NT);
  g.xsh = fold ? (4 - (num * D) % 4) % 4 : 0;
  g.k0 = fold ? num * D : 0;
  g.nxv = fold ? num : 0;
  const int need = g.k0 + g.KC0 * 32 > W0 ? g.k0 + g.KC0 * 32 : W0;
  g.WE = ((g.xsh + need + 7) & ~7) - g.xsh;  // the row's floats, xsh + WE, a multiple of 8: SE = 4 mod 8
  g.SE = g.xsh + g.WE + 4;
  g.SB = g.KCN * 32 + 8;
  return g;
}

}  // namespace

bool bf16_fused_supported(int F, int D, int H, int NT) { return D == 10 && F >= 1 && F <= kFMaxF && H >= 1 && NT >= 1 && NT <= kFW * kFTPW; }

size_t bf16_fused_lds_bytes(int rows, int F, int num, int D, int NT, int NC0, int W0, bool fold) {
  const Bf16FusedGeo g = fused_geo(F, num, D, NT, NC0, W0, fold);
  return sizeof(float) * (size_t)fused_layout(rows, F, D, NT, g.SE, g.SB).total;
}

hipError_t launch_bf16_fused(const FwdArgs& a, const uint16_t* wb, const uint16_t* wfold, int rows, hipStream_t s) {
  if (!bf16_fused_supported(a.F, 10, a.H, a.NT) || a.batch <= 0) return hipErrorInvalidValue;
  Bf16FusedGeo g = fused_geo(a.F, a.num, 10, a.NT, a.NC0, a.W0, wfold != nullptr);
  g.w1 = wfold ? wfold : wb;
  g.wn = wb + (size_t)a.NT * kc_of(a.NC0) * 64 * 8;  // behind the pack's unfolded layer 1
  const size_t lds = sizeof(float) * (size_t)fused_layout(rows, a.F, 10, a.NT, g.SE, g.SB).total;
  if (lds > kFLdsMax) return hipErrorInvalidValue;
  switch (rows) {
    case 16: return launch_rt<1>(a, g, lds, s);
    case 32: return launch_rt<2>(a, g, lds, s);
    case 64: return launch_rt<4>(a, g, lds, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_bf16_fold_pack(const float* w1, const FieldDev* fields, uint16_t* dst, int N, int F, int D, int num,
                                 int NT, hipStream_t s) {
  const int KC = bf16_fold_steps(F, num, D);
  const int64_t total = (int64_t)NT * KC * 64;
  if (total <= 0) return hipSuccess;
  hipLaunchKernelGGL(bf16_fold_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w1, fields,
                     reinterpret_cast<u32x4*>(dst), N, F, D, num, KC, total);
  return hipGetLastError();
}

}  // namespace dfwfm
