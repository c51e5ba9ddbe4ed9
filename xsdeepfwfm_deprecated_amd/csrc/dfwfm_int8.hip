// dfwfm_int8.hip -- the forward with an int8 deep tower in ONE launch (include/dfwfm_int8.h).
//
// The shape of bf16_fused_kernel (dfwfm_bf16_fused.hip): one workgroup of eight waves owns ROWS = 16 RT rows of one
// batch (RT = 1, 2) and carries them from Xi / Xv to the logits:
//
//   stage 1  descriptors, keys, the gather of the f32 E tile into LDS, the table / fwlw first order and the FwFM / FM
//            second order as U'E pieces, the fused bf16 kernel's stage 1 in its unfolded form and the same bits: the
//            gather and the first + second reduction are the stage_* functions of dfwfm_fused_stage.h that it calls
//            too, the staging and the shallow half its text again in this kernel's body (that header says why);
//   stage 2  the f32 E rows quantized into the int8 tile: TPR = 512 / ROWS lanes of one wave per row hold the row's
//            float4s in registers, take the row's max (NaN kept) by a shuffle tree, form inv = 127 / a and sx = a / 127
//            (one division each) and write four int8 per dword; sx stays in LDS;
//   stage 3  the hidden layers on v_mfma_i32_16x16x64_i8: the weights are the A operand, 16-byte fragments of the pack
//            of dfwfm_model_pack_int8 streamed from L2 (wave w owns output tiles w, w + 8, w + 16, w + 24 for every
//            row sub-tile), the activations the B operand, 16 bytes per lane from the int8 tile.  Lane l of both
//            operands holds k = 64 c + 16 (l >> 4) + 0..15 of K step c, so the integer sum is right whatever k order
//            the instruction uses inside.  The epilogue h = relu(fmaf((float)acc, sx[row] sw[n], b[n])) stays in
//            registers: every wave reduces its own tiles' max per row into LDS [row][8]; behind a barrier (which also
//            ends every wave's reads of the int8 tile) every wave combines the eight, quantizes its registers and
//            writes int8 IN PLACE of the layer's input -- no f32 round trip through LDS;
//   stage 4  the last layer's share of deep per 16-neuron tile into LDS [row][NT], the shares added in tile order,
//            logit = (first_second + deep) + bias: as the fused bf16 kernel.
//
// LDS (floats): [E tile: ROWS x SE f32][int8 tile: ROWS x SQ bytes][fs: ROWS][sx: ROWS][wmax: ROWS x 8][scratch:
// descriptors, lw, fwlw, first order, FwFM column sums -- dead after stage 1, then the last layer's shares [ROWS][NT]].
// SE = 4 mod 8 floats as in the fused bf16 kernel.  SQ = 64 max(KC0, KCN) + 16 bytes, an odd multiple of 16 (464 for
// K = 448): the sixteen rows a quarter wave reads 16 bytes of start 16 bytes apart modulo 256, no bank conflict in
// ds_read_b128.  78160 bytes at Criteo-39 with 32 rows: two workgroups per CU for both row tiles.
// The int8 tile's columns past a layer's real inputs hold zeros or an earlier layer's values; the pack's weights are 0
// there, and an integer product with 0 is 0.
// Rows past the batch hold zeros and run through every stage (every wave reaches every barrier); nothing of them is
// written out.
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

typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

// max that keeps a NaN of either side
__device__ __forceinline__ float nanmax(float a, float b) { return (b != b || b > a) ? b : a; }

// clamp(rint(x inv), -127, 127) as an integer; 0 where the product is NaN
__device__ __forceinline__ int quant1(float x, float inv) {
  float r = rintf(x * inv);
  r = r == r ? r : 0.f;
  r = fminf(fmaxf(r, -127.f), 127.f);
  return (int)r;
}
__device__ __forceinline__ uint32_t quant4(float x0, float x1, float x2, float x3, float inv) {
  return (uint32_t)(quant1(x0, inv) & 255) | (uint32_t)(quant1(x1, inv) & 255) << 8 |
         (uint32_t)(quant1(x2, inv) & 255) << 16 | (uint32_t)(quant1(x3, inv) & 255) << 24;
}

struct Int8Lds {
  int tile, qt, fs, sx, wmax, part, total;
  StageLds st;
};

__host__ __device__ inline Int8Lds int8_layout(int rows, int F, int D, int NT, int SE, int SQ) {
  Int8Lds L;
  int o = 0;
  L.tile = o;  o += r4(rows * SE);
  L.qt = o;    o += rows * SQ / 4;
  L.fs = o;    o += rows;
  L.sx = o;    o += rows;
  L.wmax = o;  o += rows * kFW;
  L.st = stage_layout(o, rows, F, D);
  const int s = L.st.end;
  int t = o;
  L.part = t;  t += rows * NT;
  L.total = r4(s > t ? s : t);
  return L;
}

// one layer's K loop of one wave: its kFTPW output tiles (wt[j]: the tile's fragments of K step 0) times the RT row
// sub-tiles (brow: this lane's 16 bytes of K step 0 in sub-tile 0; rt_bytes to the next sub-tile, 64 bytes to the next
// K step).  The weight fragment sets go through the ring of ring_k_loop; the activation fragments come from LDS in their
// own step, as in fused_k_loop of the fused bf16 kernel: the same loop on the int8 instruction.
template <int RT>
__device__ __forceinline__ void int8_k_loop(i32x4 (&acc)[RT][kFTPW], const u32x4* const (&wt)[kFTPW], int lane,
                                            const char* brow, int rt_bytes, int KC) {
  ring_k_loop<ring_depth(RT), kFTPW>(wt, lane, KC, [&](int c, const u32x4(&wq)[kFTPW]) {
    u32x4 aq[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) aq[i] = *reinterpret_cast<const u32x4*>(brow + i * rt_bytes + c * 64);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const i32x4 x = __builtin_bit_cast(i32x4, aq[i]);
#pragma unroll
      for (int j = 0; j < kFTPW; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, wq[j]), x, acc[i][j], 0, 0, 0);
    }
  });
}

// RT: 16-row sub-tiles per workgroup; QR: some field may be a QR embedding (false: the gather carries no second operand)
template <int RT, bool QR>
__global__ void __launch_bounds__(kFTH) __attribute__((amdgpu_waves_per_eu(4)))
int8_fused_kernel(const FwdArgs p, const Int8Geo q) {
  constexpr int D = 10;
  constexpr int ROWS = 16 * RT;
  constexpr int LR = RT == 1 ? 4 : 5;   // log2(ROWS)
  constexpr int TPR = kFTH / ROWS;      // lanes per row in the quantize pass: 32 or 16, inside one wave
  constexpr int Q4 = (kFMaxF * D / 4 + TPR - 1) / TPR;  // float4s per lane: layer 1's K <= 480
  static_assert(RT == 1 || RT == 2, "16 or 32 rows");
  extern __shared__ __attribute__((aligned(16))) float smem[];
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int F = p.F;
  const int flags = p.flags;
  const int Fp = r4(F);
  const int SE = q.SE, SQ = q.SQ;
  const Int8Lds L = int8_layout(ROWS, F, D, p.NT, SE, SQ);
  float* etile = smem + L.tile;
  char* qtile = reinterpret_cast<char*>(smem + L.qt);
  float* fs = smem + L.fs;
  float* sx_s = smem + L.sx;
  float* wmax = smem + L.wmax;
  const StageScratch sc = stage_scratch(smem, L.st);
  float* part = smem + L.part;
  const TileRef tr = tile_ref<ROWS>(p);  // batch set: this workgroup's batch

  // ---- stage 1: descriptors and shallow parameters to LDS, the E tile's zero padding, the int8 tile zeroed; then
  // dfwfm_fused_stage.h -------------------------------------------------------------------------------------------------
  for (int i = tid; i < 7 * F; i += kFTH)
    reinterpret_cast<u32x2*>(sc.desc)[i] = reinterpret_cast<const u32x2*>(p.fields)[i];
  if (flags & kFoFwlw)
    for (int i = tid; i < F * D; i += kFTH) sc.fwlw[i] = p.fwlw[i];
  if ((flags & kFoLw) && tid < F) sc.lw[tid] = p.lw[tid];
  {
    // columns [F D, WE): the quantize pass reads float4s up to r4(F D), the FwFM fields up to 4 S
    const int zc = F * D;
    const int w = q.WE - zc;
    for (int i = tid; i < ROWS * w; i += kFTH) {
      const int b = i / w;
      etile[b * SE + zc + (i - b * w)] = 0.f;
    }
    for (int i = tid; i < ROWS * SQ / 16; i += kFTH) reinterpret_cast<u32x4*>(qtile)[i] = u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
  stage_gather<RT, QR, false>(p, tr, sc, etile, SE, 0, tid);
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
          const int l = 4 * s + (lane >> 4);  // (the columns of fields past F are zeros)
          bv[u] = s < S ? ecol[l * D] : 0.f;
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

  // ---- stage 2: the f32 E rows to int8.  Row b = tid / TPR, its float4s c4 = sub + TPR i in registers ----------------
  {
    const int b = tid / TPR, sub = tid % TPR;
    const int n4 = (F * D + 3) / 4;  // the columns [F D, 4 n4) are zeros: they raise no max and quantize to 0
    const f32x4* erow = reinterpret_cast<const f32x4*>(etile + b * SE);
    f32x4 x[Q4];
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < Q4; ++i) {
      const int c4 = sub + TPR * i;
      x[i] = c4 < n4 ? erow[c4] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) a = nanmax(a, fabsf(x[i][r]));
    }
#pragma unroll
    for (int o = 1; o < TPR; o *= 2) a = nanmax(a, __shfl_xor(a, o));
    const float inv = a == 0.f ? 0.f : 127.f / a;
    if (sub == 0) sx_s[b] = a == 0.f ? 0.f : a / 127.f;
    uint32_t* qrow = reinterpret_cast<uint32_t*>(qtile + b * SQ);
#pragma unroll
    for (int i = 0; i < Q4; ++i) {
      const int c4 = sub + TPR * i;
      if (c4 < n4) qrow[c4] = quant4(x[i][0], x[i][1], x[i][2], x[i][3], inv);
    }
  }
  __syncthreads();

  // ---- stages 3 and 4: the hidden layers; the int8 tile is read by every wave's K loop, then overwritten in place ------
  const int rl = lane & 15, kq = lane >> 4;
  const int NT = p.NT;
  const u32x4* wl = reinterpret_cast<const u32x4*>(q.w);
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
    i32x4 acc[RT][kFTPW];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < kFTPW; ++j) acc[i][j] = i32x4{0, 0, 0, 0};
    int8_k_loop<RT>(acc, wt, lane, qtile + rl * SQ + 16 * kq, 16 * SQ, KC);
    // the lane-derived epilogue values are recomputed per layer: hoisted out of the layer loop they stay live across
    // the K loops
    int lv = lane;
    asm volatile("" : "+v"(lv));
    const int erl = lv & 15, ekq = lv >> 4;
    float sxr[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) sxr[i] = sx_s[i * 16 + erl];
    // h = relu(fmaf((float)acc, sx[row] sw[n], b[n])) in place of the accumulators (the same registers, as floats)
    f32x4 v[RT][kFTPW];
    float mx[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) mx[i] = 0.f;
#pragma unroll
    for (int j = 0; j < kFTPW; ++j) {
      const int t = wave + kFW * j;
      const bool on = t < NT;  // wave-uniform
      const int n0 = (on ? t : 0) * 16 + 4 * ekq;
      const f32x4 sq = *reinterpret_cast<const f32x4*>(q.sw + (size_t)h * NT * 16 + n0);
      const f32x4 bq = *reinterpret_cast<const f32x4*>(q.b + (size_t)h * NT * 16 + n0);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {  // padded neurons stay exactly 0
          const float t1 = sxr[i] * sq[r];
          v[i][j][r] = (on && n0 + r < p.N) ? relu_keep_nan(fmaf((float)acc[i][j][r], t1, bq[r])) : 0.f;
          mx[i] = nanmax(mx[i], v[i][j][r]);
        }
      }
    }
    if (!last) {
      // the row's max over this wave's neurons, then over all waves through LDS [row][8]
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        mx[i] = nanmax(mx[i], __shfl_xor(mx[i], 16));
        mx[i] = nanmax(mx[i], __shfl_xor(mx[i], 32));
        if (lv < 16) wmax[(i * 16 + lv) * kFW + wave] = mx[i];
      }
      __syncthreads();  // the maxes are there, and every wave has read the layer's input: the tile may be overwritten
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const int row = i * 16 + erl;
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(wmax + row * kFW);
        const f32x4 m1 = *reinterpret_cast<const f32x4*>(wmax + row * kFW + 4);
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) a = nanmax(a, m0[r]);
#pragma unroll
        for (int r = 0; r < 4; ++r) a = nanmax(a, m1[r]);
        const float inv = a == 0.f ? 0.f : 127.f / a;
        if (wave == 0 && lv < 16) sx_s[row] = a == 0.f ? 0.f : a / 127.f;
#pragma unroll
        for (int j = 0; j < kFTPW; ++j) {
          const int t = wave + kFW * j;
          if (t < NT)  // wave-uniform
            *reinterpret_cast<uint32_t*>(qtile + row * SQ + t * 16 + 4 * ekq) =
                quant4(v[i][j][0], v[i][j][1], v[i][j][2], v[i][j][3], inv);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < kFTPW; ++j) {
        const int t = wave + kFW * j;
        if (t >= NT) break;  // wave-uniform
        const f32x4 fq = *reinterpret_cast<const f32x4*>(p.fc + t * 16 + 4 * ekq);
#pragma unroll
        for (int i = 0; i < RT; ++i)  // uniform: every lane takes part in the shuffles
          last_layer_share(v[i][j], fq, lv, part + (i * 16 + lv) * NT + t);
      }
    }
    wl += (size_t)NT * KC * 64;
    __syncthreads();
  }

  // ---- logit[b] = (first_second[b] + the shares in tile order) + bias ---------------------------------------------------
  stage_logits<ROWS>(p, tr, part, fs, NT, tid);
}

// dfwfm_model_pack_int8: a workgroup per (layer, output tile of 16 neurons).  Sixteen lanes per neuron take the row's
// max |W| (a 16-lane shuffle tree that keeps a NaN: sw is then NaN and the neuron NaN for every row, never an ordinary
// zero); sw = aw / 127, or 1 for a zero row; then a thread per (K step, lane) writes its 16 weights of neuron
// n = 16 t + (l & 15), k = 64 c + 16 (l >> 4) + 0..15, as clamp(rint(W / sw), -127, 127), zero outside [N][K].  The
// tile's sw and biases (the padded f32 biases of set_dense) go beside the pack.
struct Int8PackArgs {
  const float* w[kMaxH];  // the caller's weights of the last set_dense, [N][K_l] row-major
  const float* mlp_b;     // [H][NT*16] padded biases (model-owned, written by set_dense on the stream)
  u32x4* dst;
  float* sw;              // [H][NT*16]
  float* b;               // [H][NT*16]
  int32_t H, N, K0, NT, KC0, KCN;
};

__global__ void __launch_bounds__(256) int8_pack_kernel(const Int8PackArgs a) {
  __shared__ float sw_s[16];
  const int tid = threadIdx.x;
  const int h = (int)blockIdx.x / a.NT;
  const int t = (int)blockIdx.x - h * a.NT;
  const int K = h == 0 ? a.K0 : a.N;
  const int KC = h == 0 ? a.KC0 : a.KCN;
  const float* __restrict__ w = a.w[h];
  {
    const int n = t * 16 + (tid >> 4);
    float aw = 0.f;
    if (n < a.N)
      for (int k = tid & 15; k < K; k += 16) aw = nanmax(aw, fabsf(w[(size_t)n * K + k]));
#pragma unroll
    for (int o = 1; o < 16; o *= 2) aw = nanmax(aw, __shfl_xor(aw, o));
    if ((tid & 15) == 0) {
      const float s = aw == 0.f ? 1.f : aw / 127.f;
      sw_s[tid >> 4] = s;
      a.sw[(size_t)h * a.NT * 16 + n] = s;
      a.b[(size_t)h * a.NT * 16 + n] = a.mlp_b[(size_t)h * a.NT * 16 + n];
    }
  }
  __syncthreads();
  u32x4* dst = a.dst + ((size_t)(h == 0 ? 0 : a.KC0 + (h - 1) * a.KCN) * a.NT + (size_t)t * KC) * 64;
  for (int i = tid; i < KC * 64; i += 256) {
    const int lane = i & 63;
    const int n = t * 16 + (lane & 15);
    const int k0 = (i >> 6) * 64 + 16 * (lane >> 4);
    const float s = sw_s[lane & 15];
    uint32_t d[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      int qv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = k0 + 4 * g + r;
        float x = (n < a.N && k < K) ? rintf(w[(size_t)n * K + k] / s) : 0.f;
        x = x == x ? x : 0.f;
        qv[r] = (int)fminf(fmaxf(x, -127.f), 127.f);
      }
      d[g] = (uint32_t)(qv[0] & 255) | (uint32_t)(qv[1] & 255) << 8 | (uint32_t)(qv[2] & 255) << 16 |
             (uint32_t)(qv[3] & 255) << 24;
    }
    dst[i] = u32x4{d[0], d[1], d[2], d[3]};
  }
}

template <int RT>
hipError_t launch_rt(const FwdArgs& a, const Int8Geo& g, size_t lds, hipStream_t s) {
  auto k = (a.flags & kHasQR) ? int8_fused_kernel<RT, true> : int8_fused_kernel<RT, false>;
  return launch_fused_kernel(k, a, g, 16 * RT, kFTH, lds, s);
}

inline int kc64(int cols) { return (cols + 63) / 64; }

Int8Geo int8_geo(int F, int D, int NT, int W0) {
  Int8Geo g;
  g.w = nullptr;
  g.sw = g.b = nullptr;
  g.KC0 = kc64(F * D);
  g.KCN = kc64(NT * 16);
  const int need = r4(F * D) > W0 ? r4(F * D) : W0;
  g.WE = (need + 7) & ~7;  // the row's floats a multiple of 8: SE = 4 mod 8
  g.SE = g.WE + 4;
  g.SQ = 64 * (g.KC0 > g.KCN ? g.KC0 : g.KCN) + 16;
  return g;
}

}  // namespace

bool int8_supported(int F, int D, int H, int NT) {
  return D == 10 && F >= 1 && F <= kFMaxF && H >= 1 && H <= kMaxH && NT >= 1 && NT <= kFW * kFTPW;
}

size_t int8_pack_bytes(int F, int D, int H, int NT) {
  return ((size_t)kc64(F * D) + (size_t)(H - 1) * kc64(NT * 16)) * NT * 64 * 16;
}

size_t int8_lds_bytes(int rows, int F, int D, int NT, int W0) {
  const Int8Geo g = int8_geo(F, D, NT, W0);
  return sizeof(float) * (size_t)int8_layout(rows, F, D, NT, g.SE, g.SQ).total;
}

hipError_t launch_int8_pack(const float* const* w, const float* mlp_b, int8_t* dst, float* sw, float* b, int H, int N,
                            int F, int D, int NT, hipStream_t s) {
  if (H < 1 || H > kMaxH) return hipErrorInvalidValue;
  Int8PackArgs a;
  memset(&a, 0, sizeof a);
  for (int h = 0; h < H; ++h) a.w[h] = w[h];
  a.mlp_b = mlp_b;
  a.dst = reinterpret_cast<u32x4*>(dst);
  a.sw = sw;
  a.b = b;
  a.H = H;
  a.N = N;
  a.K0 = F * D;
  a.NT = NT;
  a.KC0 = kc64(F * D);
  a.KCN = kc64(NT * 16);
  hipLaunchKernelGGL(int8_pack_kernel, dim3((unsigned)(H * NT)), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_int8_fused(const FwdArgs& a, const int8_t* w, const float* sw, const float* b, int rows,
                             hipStream_t s) {
  if (!int8_supported(a.F, 10, a.H, a.NT) || a.batch <= 0) return hipErrorInvalidValue;
  Int8Geo g = int8_geo(a.F, 10, a.NT, a.W0);
  g.w = w;
  g.sw = sw;
  g.b = b;
  const size_t lds = sizeof(float) * (size_t)int8_layout(rows, a.F, 10, a.NT, g.SE, g.SQ).total;
  if (lds > kFLdsMax) return hipErrorInvalidValue;
  switch (rows) {
    case 16: return launch_rt<1>(a, g, lds, s);
    case 32: return launch_rt<2>(a, g, lds, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace dfwfm
