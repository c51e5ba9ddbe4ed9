// dfwfm_serve.hip -- the small-batch serving forward's deep tower (include/dfwfm_serve.h).
//
// Below about 1024 rows the fused forward has fewer 16-row tiles than the chip has CUs, and each tile's layers run
// one after the other on one CU.  Here every layer is its own launch and every 16 x 16 output tile of a layer its own
// workgroup, so a lone sample's 3 x 400 tower runs on 25 workgroups per layer instead of one.  Stream order between
// the launches is the only dependency: no workgroup waits on another, there are no atomics, and every buffer written
// is in the caller's workspace.
//
// Summation order of one output element (fixed by the layer's shape alone): wave w of the workgroup's eight adds the
// tile's K chunks [NC w / 8, NC (w + 1) / 8) in ascending k on MFMA, the partial tiles are added in LDS in wave order
// (((p0 + p1) + p2) + ... + p7), then the bias.  The last hidden layer forms each tile's share of
// deep[b] = sum_n h[b, n] fc[n] (four neurons per lane by fma in ascending n, then the four lane groups as
// (q0 + q1) + (q2 + q3)) into partial[row][tile]; the combine launch adds the shares in tile order:
// logit = (first_second + deep) + bias.
// (A ticket per row tile -- the last layer's last-arriving workgroup adding the shares -- would save the combine launch,
// but its device-scope fences write back and invalidate the L2s: measured 19.1 us against 18.2 us per call at B = 1 and
// 329 against 119 us at B = 4096.)
#include "dfwfm_device.h"

namespace dfwfm {

namespace {

constexpr int kServeWaves = 8;  // K split of one output tile: a 25-chunk layer is 3 or 4 chunks = 12 or 16 dependent
                                // MFMAs per wave
constexpr int kServeCh = 4;     // K chunks a wave keeps in flight (layers of up to 32 chunks: one round)

struct ServeLayer {
  const float* in;       // [rows16][in_stride] (K zero padded to NC*16)
  float* out;            // [rows16][NT*16], or null in the last layer
  float* partial;        // [rows16][NT] in the last layer, else null
  const f32x4* w;        // [NT][NC][64] forward fragments of this layer
  const float* b;        // [NT*16]
  const float* fc;       // [NT*16]
  int64_t batch;
  int32_t in_stride, NC, NT, N;
};

// workgroup = (row tile blockIdx.x / NT, output tile blockIdx.x % NT).  Fragment algebra as fwd_kernel's (weights
// the MFMA A operand): in sub-step s of chunk c lane l supplies W[16t + (l&15)][16c + 4(l>>4) + s] and
// in[row l&15][16c + 4(l>>4) + s], and holds neurons 16t + 4(l>>4) + r of row l&15.
__global__ void __launch_bounds__(64 * kServeWaves) serve_layer_kernel(const ServeLayer a) {
  __shared__ f32x4 part[(kServeWaves - 1) * 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  const int rt = (int)blockIdx.x / a.NT;
  const int t = (int)blockIdx.x - rt * a.NT;
  const int rowl = lane & 15, nq = 4 * (lane >> 4);
  const int64_t row = (int64_t)rt * kBM + rowl;
  const bool live = row < a.batch;  // the gather launch leaves the rows past the batch unwritten
  const float* arow = a.in + row * a.in_stride + nq;
  const f32x4* wt = a.w + (size_t)t * a.NC * 64 + lane;
  const int lo = a.NC * w / kServeWaves, hi = a.NC * (w + 1) / kServeWaves;

  // wave 0's epilogue operands, ahead of the K loop (behind it they would cost a second memory round trip)
  f32x4 bq = {0.f, 0.f, 0.f, 0.f}, wf = {0.f, 0.f, 0.f, 0.f};
  if (w == 0) {
    bq = *reinterpret_cast<const f32x4*>(a.b + t * 16 + nq);
    if (a.partial) wf = *reinterpret_cast<const f32x4*>(a.fc + t * 16 + nq);
  }

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int c = lo; c < hi; c += kServeCh) {
    f32x4 wv[kServeCh], av[kServeCh];
#pragma unroll
    for (int u = 0; u < kServeCh; ++u) {
      const int cc = c + u < hi ? c + u : hi - 1;
      wv[u] = wt[cc * 64];
      av[u] = live ? *reinterpret_cast<const f32x4*>(arow + cc * 16) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int u = 0; u < kServeCh; ++u) {
      if (c + u < hi) {  // wave-uniform
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].x, av[u].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].y, av[u].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].z, av[u].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u].w, av[u].w, acc, 0, 0, 0);
      }
    }
  }
  if (w > 0) part[(w - 1) * 64 + lane] = acc;
  __syncthreads();
  if (w > 0) return;
#pragma unroll
  for (int k = 0; k < kServeWaves - 1; ++k) acc += part[k * 64 + lane];  // wave order 0, 1, ..., 7

  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r)  // padded neurons stay exactly 0
    v[r] = t * 16 + nq + r < a.N ? relu_keep_nan(acc[r] + bq[r]) : 0.f;
  if (a.out) *reinterpret_cast<f32x4*>(a.out + row * ((int64_t)a.NT * 16) + t * 16 + nq) = v;
  if (a.partial) {
    float d = 0.f;
    d = fmaf(v[0], wf[0], d);
    d = fmaf(v[1], wf[1], d);
    d = fmaf(v[2], wf[2], d);
    d = fmaf(v[3], wf[3], d);
    d += __shfl_xor(d, 16);
    d += __shfl_xor(d, 32);
    if (lane < 16) a.partial[row * a.NT + t] = d;
  }
}

// logit[b] = (first_second[b] + sum over tiles, in tile order, of partial[b][tile]) + bias
__global__ void __launch_bounds__(256) serve_combine_kernel(const float* __restrict__ partial,
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

}  // namespace

// deep_emb | first + second | two activation buffers | partials, for ceil(batch / 16) * 16 rows (every region a
// multiple of 16 floats)
size_t serve_workspace_floats(int NT, int NC0, int64_t batch) {
  const size_t rows16 = (size_t)((batch + kBM - 1) / kBM) * kBM;
  return rows16 * ((size_t)NC0 * 16 + 1 + 2 * (size_t)NT * 16 + (size_t)NT);
}

hipError_t launch_serve_mlp(const ServeArgs& a, hipStream_t s) {
  const int64_t tiles = (a.batch + kBM - 1) / kBM;
  if (a.batch <= 0 || a.H < 1 || tiles * a.NT > 0x7fffffff) return hipErrorInvalidValue;
  size_t woff = 0;  // float4 offset of the layer in wpack
  for (int h = 0; h < a.H; ++h) {
    const bool last = h == a.H - 1;
    ServeLayer l;
    l.in = h == 0 ? a.deep_emb : a.act[(h - 1) & 1];
    l.in_stride = h == 0 ? a.NC0 * 16 : a.NT * 16;
    l.NC = h == 0 ? a.NC0 : a.NT;
    l.out = last ? nullptr : a.act[h & 1];
    l.partial = last ? a.partial : nullptr;
    l.w = reinterpret_cast<const f32x4*>(a.wpack) + woff;
    l.b = a.mlp_b + (size_t)h * a.NT * 16;
    l.fc = a.fc;
    l.batch = a.batch;
    l.NT = a.NT;
    l.N = a.N;
    hipLaunchKernelGGL(serve_layer_kernel, dim3((unsigned)(tiles * a.NT)), dim3(64 * kServeWaves), 0, s, l);
    woff += (size_t)a.NT * l.NC * 64;
  }
  hipLaunchKernelGGL(serve_combine_kernel, dim3((unsigned)((a.batch + 255) / 256)), dim3(256), 0, s, a.partial, a.fs,
                     a.bias, a.out, a.batch, a.NT);
  return hipGetLastError();
}

}  // namespace dfwfm
