// dfwfm_bf16.hip -- the bf16 deep tower of the inference forward (include/dfwfm_bf16.h states the numeric contract).
//
// The hidden layers run on v_mfma_f32_16x16x32_bf16 with f32 accumulation, one launch per layer behind the gather
// launch (which writes the f32 E rows and first + second order), then a combine launch.  Stream order between the
// launches is the only dependency: no atomics, no workgroup waits on another, every buffer written is in the
// caller's workspace.
//
// Operands (weights the MFMA A operand, activations B, as in the f32 kernels' WA form): in K step c lane l supplies
// Wb[16t + (l&15)][32c + 8(l>>4) + j] and x[row l&15][32c + 8(l>>4) + j], j = 0..7 -- one 16-byte load each, the
// weights from the pack [NT][KC][64 lanes][8 bf16] (zero for neurons >= N and k >= K), the activations from the
// row-major bf16 buffer of the layer before (layer 0: two 16-byte loads of the f32 E row, rounded to bf16 on the
// way).  The accumulator of lane l holds neurons 16t + 4(l>>4) + r, r = 0..3, of row l&15: four consecutive bf16
// outputs are one 8-byte store.
//
// Summation order of one output element (fixed by the layer's shape alone): one accumulator takes the K steps
// c = 0, 1, ..., KC - 1 in turn, whatever the tile a wave carries (RT x CT 16 x 16 tiles: the shapes differ only
// in how many rows and neurons share a fragment load, where the weight fragments come from (L2, or an LDS copy) and
// how far ahead the fragments are fetched; launch_bf16_mlp chooses from the batch size).  The last hidden layer forms
// each 16-neuron tile's share of deep[b] = sum_n h[b, n] fc[n] (four neurons per lane by fma in ascending n, then
// the four lane groups as (q0 + q1) + (q2 + q3)) into partial[row][tile]; the combine launch adds the shares in tile
// order: logit = (first_second + deep) + bias.
#include "dfwfm_device.h"

namespace dfwfm {

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kBf16Waves = 4;  // waves of a workgroup: consecutive row blocks of one column block
constexpr size_t kBf16SlabMax = 80 * 1024;  // LDS of the slab form's weight block: two workgroups share a CU's 160 KiB

// two f32 to two bf16, round to nearest even, NaN kept: lo in bits 0-15
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  uint32_t r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(lo), "v"(hi));
  return r;
}

// Workgroups are dealt to the 8 XCDs in turn (workgroup b runs on XCD b % 8), each with an L2 of its own.  The column
// blocks of one row group read the same activation rows, so they should share an L2: xcd_order gives workgroup b a
// position such that consecutive positions run on one XCD (XCD x takes positions [x n / 8, (x + 1) n / 8), the
// first n % 8 XCDs one more).  Without it every activation row came from beyond the L2 once per column block.
__device__ __forceinline__ int64_t xcd_order(int64_t b, int64_t n) {
  const int64_t q = n / 8, r = n % 8, x = b % 8, i = b / 8;
  return x < r ? x * (q + 1) + i : r * (q + 1) + (x - r) * q + i;
}

struct Bf16Layer {
  const void* in;      // layer 0: f32 [rows][in_stride], else bf16 [rows][in_stride]
  uint16_t* out;       // bf16 [rows][NT*16], or null in the last layer
  float* partial;      // [rows][NT] in the last layer, else null
  const u32x4* w;      // [NT][KC][64] fragments of this layer
  const float* b;      // [NT*16]
  const float* fc;     // [NT*16]
  int64_t batch;
  int64_t nrb;         // row blocks of 16 * RT rows
  int32_t in_stride;   // elements
  int32_t in_cols;     // columns of `in` that hold data (a multiple of 16); K steps read zeros past them
  int32_t KC, NT, N, ncb;
  int32_t ngroups;     // slab kernel: workgroups per column block (row blocks are dealt round robin)
};

// the B fragment of one 16-row tile: raw as loaded (f32: 8 floats, bf16: 8 halves), converted at the MFMA.  The load
// is unconditional (a predicated load is a branch, and the waits behind a branch cover every load in flight): the
// caller clamps the address into the buffer and `ok` zeroes the fragment when it is used
template <bool F32IN>
struct ActFrag;
template <>
struct ActFrag<true> {
  f32x4 lo, hi;
  bool ok;
  __device__ __forceinline__ void load(const void* p, bool ok_) {
    lo = reinterpret_cast<const f32x4*>(p)[0];
    hi = reinterpret_cast<const f32x4*>(p)[1];
    ok = ok_;
  }
  __device__ __forceinline__ bf16x8 get() const {
    const u32x4 v = {cvt_pk_bf16(lo[0], lo[1]), cvt_pk_bf16(lo[2], lo[3]), cvt_pk_bf16(hi[0], hi[1]),
                     cvt_pk_bf16(hi[2], hi[3])};
    return __builtin_bit_cast(bf16x8, ok ? v : u32x4{0u, 0u, 0u, 0u});
  }
  static constexpr int kElem = 4;
};
template <>
struct ActFrag<false> {
  u32x4 v;
  bool ok;
  __device__ __forceinline__ void load(const void* p, bool ok_) {
    v = *reinterpret_cast<const u32x4*>(p);
    ok = ok_;
  }
  __device__ __forceinline__ bf16x8 get() const { return __builtin_bit_cast(bf16x8, ok ? v : u32x4{0u, 0u, 0u, 0u}); }
  static constexpr int kElem = 2;
};

// bias, relu, and the layer's output of one wave's RT x CT tiles: bf16 activations for the next layer, or in the last
// layer each tile's share of deep[b]
template <int RT, int CT>
__device__ __forceinline__ void layer_epilogue(const Bf16Layer& a, const f32x4 (&acc)[RT][CT], const bool (&live)[RT],
                                               int64_t rb, int t0, int lane) {
  const int rl = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int t = t0 + j;
    if (t >= a.NT) break;  // wave-uniform
    const int n0 = t * 16 + 4 * kq;
    const f32x4 bq = *reinterpret_cast<const f32x4*>(a.b + n0);
    f32x4 fq = {0.f, 0.f, 0.f, 0.f};
    if (a.partial) fq = *reinterpret_cast<const f32x4*>(a.fc + n0);
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int64_t row = (rb * RT + i) * 16 + rl;
      f32x4 v;
#pragma unroll
      for (int r = 0; r < 4; ++r)  // padded neurons stay exactly 0
        v[r] = n0 + r < a.N ? relu_keep_nan(acc[i][j][r] + bq[r]) : 0.f;
      if (a.out && live[i])
        *reinterpret_cast<u32x2*>(a.out + row * ((int64_t)a.NT * 16) + n0) =
            u32x2{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3])};
      if (a.partial) {  // uniform: every lane takes part in the shuffles
        float d = 0.f;
        d = fmaf(v[0], fq[0], d);
        d = fmaf(v[1], fq[1], d);
        d = fmaf(v[2], fq[2], d);
        d = fmaf(v[3], fq[3], d);
        d += __shfl_xor(d, 16);
        d += __shfl_xor(d, 32);
        if (lane < 16 && live[i]) a.partial[row * a.NT + t] = d;
      }
    }
  }
}

// wave = (row block of 16 RT rows, column block of CT 16-neuron tiles); workgroup = kBf16Waves consecutive row
// blocks of one column block, or (COLW) every column block of one row block.  Rows past the batch are never read or
// written: their lanes re-read row 0, and what they compute (a column of the MFMA result per row, independent of the
// others) is dropped.
// COLW: the workgroup is one row block and its waves are the column blocks (at most 8), so the waves fetch the same
// activation fragments at about the same time and all but the first find them in the CU's L1.
template <int RT, int CT, int PD, bool F32IN, bool COLW>
__global__ void __launch_bounds__(COLW ? 512 : 64 * kBf16Waves) bf16_layer_kernel(const Bf16Layer a) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  int64_t rb;
  int cb;
  if constexpr (COLW) {
    rb = blockIdx.x;
    cb = wv;
  } else {
    const int64_t pos = xcd_order(blockIdx.x, gridDim.x);
    const int64_t g = pos / a.ncb;
    cb = (int)(pos - g * a.ncb);
    rb = g * kBf16Waves + wv;
  }
  if (rb >= a.nrb || cb >= a.ncb) return;  // no barrier below
  const int rl = lane & 15, kq = lane >> 4;
  const int t0 = cb * CT;

  const char* arow[RT];
  bool live[RT];
#pragma unroll
  for (int i = 0; i < RT; ++i) {
    const int64_t row = (rb * RT + i) * 16 + rl;
    live[i] = row < a.batch;
    arow[i] = static_cast<const char*>(a.in) + (live[i] ? row : 0) * a.in_stride * ActFrag<F32IN>::kElem;
  }
  const u32x4* wt[CT];
#pragma unroll
  for (int j = 0; j < CT; ++j) {
    const int t = t0 + j < a.NT ? t0 + j : a.NT - 1;  // clamped duplicates, results discarded
    wt[j] = a.w + (size_t)t * a.KC * 64 + lane;
  }

  f32x4 acc[RT][CT];
#pragma unroll
  for (int i = 0; i < RT; ++i)
#pragma unroll
    for (int j = 0; j < CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // PD fragment sets in a ring, each loaded PD - 1 K steps ahead of its MFMAs (a wave or two per SIMD cannot hide
  // the L2 round trip of a step behind the step before it); the loop is unrolled by PD so no set is ever copied
  u32x4 wf[PD][CT];
  ActFrag<F32IN> af[PD][RT];
  auto load = [&](int c, u32x4(&wq)[CT], ActFrag<F32IN>(&aq)[RT]) {
#pragma unroll
    for (int j = 0; j < CT; ++j) wq[j] = wt[j][(size_t)c * 64];
    const int k = c * 32 + 8 * kq;  // past the row's data (half of an odd layer's last K step): re-read, then zeroed
    const int kin = k < a.in_cols ? k : a.in_cols - 8;
#pragma unroll
    for (int i = 0; i < RT; ++i) aq[i].load(arow[i] + kin * ActFrag<F32IN>::kElem, k < a.in_cols);
  };
  auto mma = [&](const u32x4(&wq)[CT], const ActFrag<F32IN>(&aq)[RT]) {
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const bf16x8 x = aq[i].get();
#pragma unroll
      for (int j = 0; j < CT; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq[j]), x, acc[i][j], 0, 0, 0);
    }
  };
#pragma unroll
  for (int p = 0; p < PD - 1; ++p)
    if (p < a.KC) load(p, wf[p], af[p]);
  int c = 0;
  for (; c + 2 * PD - 1 <= a.KC; c += PD) {  // steady state: every step's refill is in range
#pragma unroll
    for (int p = 0; p < PD; ++p) {
      load(c + p + PD - 1, wf[(p + PD - 1) % PD], af[(p + PD - 1) % PD]);
      mma(wf[p], af[p]);
      __builtin_amdgcn_sched_barrier(0);  // the refill stays ahead of the step's MFMAs (hipcc sinks it to its use)
    }
  }
  for (; c < a.KC; c += PD) {  // the last 1 .. 2 PD - 2 steps (conditions wave-uniform)
#pragma unroll
    for (int p = 0; p < PD; ++p) {
      if (c + p < a.KC) {
        if (c + p + PD - 1 < a.KC) load(c + p + PD - 1, wf[(p + PD - 1) % PD], af[(p + PD - 1) % PD]);
        mma(wf[p], af[p]);
      }
    }
  }

  layer_epilogue<RT, CT>(a, acc, live, rb, t0, lane);
}

// The same layer for large batches: the workgroup's column block of the pack -- all K steps of its CT tiles, CT KC KiB
// -- is copied into LDS once, and each of its waves then carries 32-row blocks (rb = first, first + stride, ...)
// through it, fetching only the activations from global memory (PD sets ahead) and the weight fragments by
// ds_read_b128 one K step ahead.  The pack's fragment order makes the LDS image conflict-free as it is.  One barrier,
// behind the copy.  The same sums in the same order as bf16_layer_kernel.
template <int PD, bool F32IN>
__global__ void __launch_bounds__(64 * kBf16Waves) bf16_layer_slab_kernel(const Bf16Layer a) {
  constexpr int RT = 2, CT = 5;
  static_assert(PD % 2 == 0, "the two weight sets alternate with the K step");
  extern __shared__ __attribute__((aligned(16))) u32x4 slab[];  // [CT][KC][64]
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int pos = (int)xcd_order(blockIdx.x, gridDim.x);
  const int g = pos / a.ncb;
  const int cb = pos - g * a.ncb;
  const int t0 = cb * CT;
  const int per = a.KC * 64;
  for (int i = threadIdx.x; i < CT * per; i += 64 * kBf16Waves) {
    const int j = i / per;
    const int t = t0 + j < a.NT ? t0 + j : a.NT - 1;  // clamped duplicates, results discarded
    slab[i] = a.w[(size_t)t * per + (i - j * per)];
  }
  __syncthreads();
  const int rl = lane & 15, kq = lane >> 4;
  const u32x4* ws_base = slab + lane;
  for (int64_t rb = (int64_t)g * kBf16Waves + wv; rb < a.nrb; rb += (int64_t)a.ngroups * kBf16Waves) {
    const char* arow[RT];
    bool live[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      const int64_t row = (rb * RT + i) * 16 + rl;
      live[i] = row < a.batch;
      arow[i] = static_cast<const char*>(a.in) + (live[i] ? row : 0) * a.in_stride * ActFrag<F32IN>::kElem;
    }
    f32x4 acc[RT][CT];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 ws[2][CT];
    ActFrag<F32IN> af[PD][RT];
    auto aload = [&](int c, ActFrag<F32IN>(&aq)[RT]) {
      const int k = c * 32 + 8 * kq;  // past the row's data (half of an odd layer's last K step): re-read, then zeroed
      const int kin = k < a.in_cols ? k : a.in_cols - 8;
#pragma unroll
      for (int i = 0; i < RT; ++i) aq[i].load(arow[i] + kin * ActFrag<F32IN>::kElem, k < a.in_cols);
    };
    auto wload = [&](int c, u32x4(&wq)[CT]) {
#pragma unroll
      for (int j = 0; j < CT; ++j) wq[j] = ws_base[(j * a.KC + c) * 64];
    };
    auto mma = [&](const u32x4(&wq)[CT], const ActFrag<F32IN>(&aq)[RT]) {
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const bf16x8 x = aq[i].get();
#pragma unroll
        for (int j = 0; j < CT; ++j)
          acc[i][j] =
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wq[j]), x, acc[i][j], 0, 0, 0);
      }
    };
#pragma unroll
    for (int p = 0; p < PD - 1; ++p)
      if (p < a.KC) aload(p, af[p]);
    wload(0, ws[0]);
    int c = 0;  // a multiple of PD (even): step c + p uses weight set p & 1
    for (; c + 2 * PD - 1 <= a.KC; c += PD) {
#pragma unroll
      for (int p = 0; p < PD; ++p) {
        aload(c + p + PD - 1, af[(p + PD - 1) % PD]);
        wload(c + p + 1, ws[(p + 1) & 1]);
        mma(ws[p & 1], af[p]);
        __builtin_amdgcn_sched_barrier(0);  // the refills stay ahead of the step's MFMAs
      }
    }
    for (; c < a.KC; c += PD) {
#pragma unroll
      for (int p = 0; p < PD; ++p) {
        if (c + p < a.KC) {
          if (c + p + PD - 1 < a.KC) aload(c + p + PD - 1, af[(p + PD - 1) % PD]);
          if (c + p + 1 < a.KC) wload(c + p + 1, ws[(p + 1) & 1]);
          mma(ws[p & 1], af[p]);
        }
      }
    }
    layer_epilogue<RT, CT>(a, acc, live, rb, t0, lane);
  }
}

// logit[b] = (first_second[b] + sum over tiles, in tile order, of partial[b][tile]) + bias
__global__ void __launch_bounds__(256) bf16_combine_kernel(const float* __restrict__ partial,
                                                           const float* __restrict__ fs,
                                                           const float* __restrict__ bias, float* __restrict__ out,
                                                           int64_t batch, int NT) {
  const int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (b >= batch) return;
  const float* p = partial + b * NT;
  float deep = p[0];
  for (int t = 1; t < NT; ++t) deep += p[t];
  out[b] = (fs[b] + deep) + bias[0];
}

// one thread per (tile, K step, lane): its 8 weights W[16t + (l&15)][32c + 8(l>>4) + j] as bf16, zero outside [N][K]
__global__ void __launch_bounds__(256) bf16_pack_kernel(const float* __restrict__ w, u32x4* __restrict__ dst, int N,
                                                        int K, int KC, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int lane = (int)(i & 63);
  const int64_t tc = i >> 6;
  const int c = (int)(tc % KC);
  const int n = (int)(tc / KC) * 16 + (lane & 15);
  const int k0 = c * 32 + 8 * (lane >> 4);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (n < N && k0 + j < K) ? w[(size_t)n * K + k0 + j] : 0.f;
  dst[i] = u32x4{cvt_pk_bf16(v[0], v[1]), cvt_pk_bf16(v[2], v[3]), cvt_pk_bf16(v[4], v[5]), cvt_pk_bf16(v[6], v[7])};
}

template <int RT, int CT, int PD>
hipError_t launch_layer(Bf16Layer& l, bool f32in, hipStream_t s) {
  l.nrb = (l.batch + 16 * RT - 1) / (16 * RT);
  l.ncb = (l.NT + CT - 1) / CT;
  if constexpr (CT > 1) {  // a workgroup per row block, a wave per column block (deep_nodes <= 512: at most 7)
    if (l.nrb > 0x7fffffff || l.ncb > 8) return hipErrorInvalidValue;
    const dim3 grid((unsigned)l.nrb), block(64 * l.ncb);
    if (f32in)
      hipLaunchKernelGGL((bf16_layer_kernel<RT, CT, PD, true, true>), grid, block, 0, s, l);
    else
      hipLaunchKernelGGL((bf16_layer_kernel<RT, CT, PD, false, true>), grid, block, 0, s, l);
  } else {  // four row blocks of one column block
    const int64_t blocks = (l.nrb + kBf16Waves - 1) / kBf16Waves * l.ncb;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks), block(64 * kBf16Waves);
    if (f32in)
      hipLaunchKernelGGL((bf16_layer_kernel<RT, CT, PD, true, false>), grid, block, 0, s, l);
    else
      hipLaunchKernelGGL((bf16_layer_kernel<RT, CT, PD, false, false>), grid, block, 0, s, l);
  }
  return hipSuccess;
}

// the slab form: two workgroups per CU's worth of row groups per column block at most
// (PDF / PDB: activation sets in flight from the f32 E rows / from bf16 activations; the f32 rows take twice the
// registers, and two waves must fit a SIMD)
template <int PDF, int PDB>
hipError_t launch_layer_slab(Bf16Layer& l, bool f32in, hipStream_t s) {
  l.nrb = (l.batch + 31) / 32;
  l.ncb = (l.NT + 4) / 5;
  const int64_t wgs = (l.nrb + kBf16Waves - 1) / kBf16Waves;
  const int64_t cap = 512 / l.ncb > 0 ? 512 / l.ncb : 1;
  l.ngroups = (int32_t)(wgs < cap ? wgs : cap);
  const size_t lds = (size_t)5 * l.KC * 64 * sizeof(u32x4);
  const void* fn = f32in ? reinterpret_cast<const void*>(&bf16_layer_slab_kernel<PDF, true>)
                         : reinterpret_cast<const void*>(&bf16_layer_slab_kernel<PDB, false>);
  const hipError_t e = ensure_lds_limit(fn, lds);
  if (e != hipSuccess) return e;
  const dim3 grid((unsigned)(l.ngroups * l.ncb));
  if (f32in)
    hipLaunchKernelGGL((bf16_layer_slab_kernel<PDF, true>), grid, dim3(64 * kBf16Waves), lds, s, l);
  else
    hipLaunchKernelGGL((bf16_layer_slab_kernel<PDB, false>), grid, dim3(64 * kBf16Waves), lds, s, l);
  return hipSuccess;
}

inline int kc_of(int cols16) { return (cols16 * 16 + 31) / 32; }

}  // namespace

size_t bf16_pack_elems(int H, int NT, int NC0) {
  return ((size_t)NT * kc_of(NC0) + (size_t)(H - 1) * NT * kc_of(NT)) * 64 * 8;
}

// f32 deep_emb | first + second | partials | two bf16 activation buffers, for ceil(batch / 16) * 16 rows
size_t bf16_workspace_bytes(int NT, int NC0, int64_t batch) {
  const size_t rows16 = (size_t)((batch + kBM - 1) / kBM) * kBM;
  return rows16 * (sizeof(float) * ((size_t)NC0 * 16 + 1 + (size_t)NT) + 2 * sizeof(uint16_t) * (size_t)NT * 16);
}

hipError_t launch_bf16_pack(const float* const* w, uint16_t* wb, int H, int N, int K0, int NT, int NC0,
                            hipStream_t s) {
  u32x4* dst = reinterpret_cast<u32x4*>(wb);
  for (int h = 0; h < H; ++h) {
    const int KC = kc_of(h == 0 ? NC0 : NT);
    const int64_t total = (int64_t)NT * KC * 64;
    hipLaunchKernelGGL(bf16_pack_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, w[h], dst, N,
                       h == 0 ? K0 : N, KC, total);
    dst += total;
  }
  return hipGetLastError();
}

hipError_t launch_bf16_mlp(const Bf16Args& a, hipStream_t s) {
  if (a.batch <= 0 || a.H < 1) return hipErrorInvalidValue;
  // the form of the layer launch, by the waves a layer then has (measured at Criteo-39):
  // 0: a wave per 16 x 16 tile; 1: per 16 x 80, from 512 such waves; 2: per 32 x 80, from 1024; 3: 32 x 80 with
  // the weights in LDS, from 4096.  The sums do not depend on it; DFWFM_DIAG bf16tile=0..3 forces one
  const int cb5 = (a.NT + 4) / 5;
  const int64_t r16 = (a.batch + 15) / 16, w32 = (r16 + 1) / 2 * cb5;
  int shape = w32 >= 4096 ? 3 : (w32 >= 1024 ? 2 : (r16 * cb5 >= 512 ? 1 : 0));
  shape = diag_opt("bf16tile", shape);
  const u32x4* w = reinterpret_cast<const u32x4*>(a.wb);
  for (int h = 0; h < a.H; ++h) {
    const bool last = h == a.H - 1;
    Bf16Layer l = {};
    l.in = h == 0 ? static_cast<const void*>(a.deep_emb) : static_cast<const void*>(a.act[(h - 1) & 1]);
    l.in_stride = h == 0 ? a.NC0 * 16 : a.NT * 16;
    l.in_cols = l.in_stride;
    l.KC = kc_of(h == 0 ? a.NC0 : a.NT);
    l.out = last ? nullptr : a.act[h & 1];
    l.partial = last ? a.partial : nullptr;
    l.w = w;
    l.b = a.mlp_b + (size_t)h * a.NT * 16;
    l.fc = a.fc;
    l.batch = a.batch;
    l.NT = a.NT;
    l.N = a.N;
    const bool slab = shape == 3 && (size_t)5 * l.KC * 1024 <= kBf16SlabMax;  // else the layer's K is too long
    const hipError_t e = slab         ? launch_layer_slab<2, 4>(l, h == 0, s)
                         : shape >= 2 ? launch_layer<2, 5, 3>(l, h == 0, s)
                         : shape == 1 ? launch_layer<1, 5, 4>(l, h == 0, s)
                                      : launch_layer<1, 1, 6>(l, h == 0, s);
    if (e != hipSuccess) return e;
    w += (size_t)a.NT * l.KC * 64;
  }
  hipLaunchKernelGGL(bf16_combine_kernel, dim3((unsigned)((a.batch + 255) / 256)), dim3(256), 0, s, a.partial, a.fs,
                     a.bias, a.out, a.batch, a.NT);
  return hipGetLastError();
}

}  // namespace dfwfm
