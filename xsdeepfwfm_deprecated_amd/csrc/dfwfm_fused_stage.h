// dfwfm_fused_stage.h -- what the one-launch forwards share (dfwfm_bf16_fused.hip, dfwfm_int8.hip): the workgroup
// shape, the stage-1 scratch in LDS, stage 1 itself (Xi / Xv to the f32 E tile and first + second order), the weight
// fragment ring of a hidden layer's K loop, the last layer's shares and the logits, and the launch.
//
// Stage 1 is the arithmetic of the gather launch (fwd_kernel PART 3 with kP3Pieces) per 16-row sub-tile, so first +
// second are the bits dfwfm_forward_gather writes.  It comes in pieces that hold NO barrier: the kernels place one
// between each piece and the next, so every barrier stays visible in the kernel body (every wave reaches every one):
//
//   (kernel body)  descriptors, lw, fwlw to LDS; the E tile's columns [F D, WE) zeroed            -- barrier --
//   stage_gather   reads the descriptors; writes the E rows (FOLD: Xv behind column F D) and fo   -- barrier --
//   (kernel body)  reads E, fwlw; overwrites fo (fwlw first order), writes part2 (FwFM)           -- barrier --
//   stage_fs       reads fo, lw, part2; writes fs (read in stage_logits, behind the layers' barriers)
//
// Two pieces stay in each kernel's body, the same text twice (profiles/fused_stage/README.md has the figures).  hipcc
// optimises a function of this header on its own before it inlines it, which it never did to the kernels' own bodies:
//   - the shallow half (fwlw first order, FwFM): alone, its accumulators acc[kFMT] become one 12-register vector that
//     is copied around every MFMA -- 6 more VGPRs in the 16-row int8 kernel and 11 % on its latency;
//   - the parameter staging and zero padding, fifteen lines: as a function it left the 16-row int8 kernel with a
//     20-byte scratch frame (a spill slot the register allocator made and no longer used) where it had none.
//
// FOLD (the bf16 kernel's folded layer 1, include/dfwfm_bf16_fold.h): etile arrives shifted by xsh and the gather's
// numerical rows also store their Xv behind column F D.  The int8 kernel instantiates FOLD = false.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dfwfm_device.h"
#include "dfwfm_internal.h"

namespace dfwfm {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

constexpr int kFW = 8;            // waves of a workgroup
constexpr int kFTH = 64 * kFW;
constexpr int kFTPW = 4;          // output tiles per wave: deep_nodes <= 8 * 4 * 16 = 512
constexpr int kFMaxF = 48;        // fields: three FwFM row tiles, as the pieces form of the gather launch
constexpr int kFMT = 3;
constexpr int kFPD = 3;           // fragment sets in flight in the K loop
constexpr size_t kFLdsMax = 160 * 1024;
// 32 and 64 rows: twice / four times the accumulators, one set fewer
constexpr int ring_depth(int RT) { return RT == 1 ? kFPD : kFPD - 1; }

// the stage-1 scratch (offsets in floats): descriptors, lw, fwlw, first order, FwFM column sums -- dead after stage 1
struct StageLds {
  int desc, lw, fwlw, fo, part2, end;
};

// lays the scratch out from float offset s; .end is the first float behind it
__host__ __device__ inline StageLds stage_layout(int s, int rows, int F, int D) {
  StageLds L;
  L.desc = s;  s += r4(14 * F);
  L.lw = s;    s += r4(F);
  L.fwlw = s;  s += r4(F * D);
  L.fo = s;    s += rows * r4(F);
  L.part2 = s; s += rows * D;  // per 16-row sub-tile, its 16 D column sums
  L.end = s;
  return L;
}

struct StageScratch {
  FieldDev* desc;
  float *lw, *fwlw, *fo, *part2;
};

__device__ __forceinline__ StageScratch stage_scratch(float* smem, const StageLds L) {
  return StageScratch{reinterpret_cast<FieldDev*>(smem + L.desc), smem + L.lw, smem + L.fwlw, smem + L.fo,
                      smem + L.part2};
}

// ---- the gather: E rows and the table first order, RPT rows per thread and pass ------------------------------------
// QR: some field may be a QR embedding (false: the gather carries no second operand)
template <int RT, bool QR, bool FOLD>
__device__ __forceinline__ void stage_gather(const FwdArgs& p, const TileRef tr, const StageScratch sc, float* etile,
                                             int SE, int nxv, int tid) {
  constexpr int D = 10;
  constexpr int ROWS = 16 * RT;
  constexpr int LR = RT == 1 ? 4 : (RT == 2 ? 5 : 6);  // log2(ROWS)
  constexpr int RPT = RT == 1 ? 2 : 3;                  // gather rows per thread and pass
  constexpr int NPASS = (ROWS * kFMaxF + kFTH * RPT - 1) / (kFTH * RPT);
  const int F = p.F;
  const int num = p.num;
  const int flags = p.flags;
  const int Fp = r4(F);
  const int64_t b0 = tr.b0;
  const FieldDev* desc = sc.desc;
  float* fo = sc.fo;
  const bool needE = (flags & kNeedE) != 0;
  const bool fo_tab = (flags & kFoTables) != 0;
  constexpr int RQ = QR ? RPT : 1;
#pragma unroll 1
  for (int pass = 0; pass < NPASS; ++pass) {
    const float* pa[RPT];
    const float* pb[RQ];
    const float* qa[RPT];
    const float* qb[RQ];
    float scale[RPT];
    int mode[RPT];
    bool live[RPT], pkrow[RPT];
    int64_t key[RPT];  // gather row r -> field f = r / ROWS, sample b = r % ROWS: index or Xv bits
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int r = tid + (pass * RPT + k) * kFTH;
      const int f = r >> LR;
      const int64_t gb = b0 + (r & (ROWS - 1));
      live[k] = f < F && gb < p.batch;
      key[k] = 0;
      if (live[k]) {
        if (f < num)
          key[k] = __float_as_int(tr.xv[gb * p.xv_stride + f]);
        else
          key[k] = tr.xi[gb * p.xi_stride + (f - num)];
      }
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int r = tid + (pass * RPT + k) * kFTH;
      const int f = r >> LR;
      pa[k] = qa[k] = nullptr;
      if constexpr (QR) pb[k] = qb[k] = nullptr;
      scale[k] = 1.f;
      mode[k] = 0;
      pkrow[k] = false;
      if (!live[k]) continue;
      const FieldDev fd = desc[f];
      if (f < num) {
        scale[k] = __int_as_float((int)key[k]);
        pa[k] = fd.emb2;
        qa[k] = fd.emb1;
      } else {
        int64_t idx = key[k];
        if (idx < 0 || idx >= fd.n) {
          atomicOr(p.err, DFWFM_FLAG_INDEX_OUT_OF_RANGE);
          idx = 0;
        }
        if (!QR && p.pkw != 0) {  // the serving copy: second and first order in one aligned row
          pkrow[k] = true;
          pa[k] = p.pk[f] + idx * p.pkw;
        } else if (!QR || fd.c == 0) {
          pa[k] = fd.emb2 + idx * D;
          if (fo_tab) qa[k] = fd.emb1 + idx;
        } else if constexpr (QR) {
          const int64_t qq = idx / fd.c;
          const int64_t rr = idx - qq * fd.c;
          mode[k] = fd.op == 0 ? 1 : 2;
          pa[k] = fd.emb2 + qq * D;
          pb[k] = fd.emb2_r + rr * D;
          if (fo_tab) {
            qa[k] = fd.emb1 + qq;
            qb[k] = fd.emb1_r + rr;
          }
        }
      }
    }
    float va[RPT][D], vb[RQ][D], fa[RPT], fb[RQ];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      fa[k] = 0.f;
#pragma unroll
      for (int d = 0; d < D; ++d) va[k][d] = 0.f;
      if constexpr (QR) {
        fb[k] = 0.f;
#pragma unroll
        for (int d = 0; d < D; ++d) vb[k][d] = 0.f;
      }
      if (live[k] && pkrow[k]) {
        load_row_pk<D>(va[k], fa[k], pa[k], p.pkh);
      } else {
        if (live[k] && needE) {
          load_row<D>(va[k], pa[k]);
          if constexpr (QR)
            if (mode[k] != 0) load_row<D>(vb[k], pb[k]);
        }
        if (live[k] && fo_tab) {
          fa[k] = *qa[k];
          if constexpr (QR)
            if (mode[k] != 0) fb[k] = *qb[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
      const int r = tid + (pass * RPT + k) * kFTH;
      const int f = r >> LR;
      const int b = r & (ROWS - 1);
      if (f < F) {
        if (needE) {
          float e[D];
#pragma unroll
          for (int d = 0; d < D; ++d)
            e[d] = live[k] ? combine(mode[k], va[k][d], QR ? vb[QR ? k : 0][d] : 0.f, scale[k]) : 0.f;
          store_row<D>(etile + b * SE + f * D, e);
          if (FOLD && f < nxv) etile[b * SE + F * D + f] = live[k] ? scale[k] : 0.f;  // the folded layer 1's K row
        }
        fo[b * Fp + f] = live[k] ? combine(mode[k], fa[k], QR ? fb[QR ? k : 0] : 0.f, scale[k]) : 0.f;
      }
    }
  }
}

// first[b] (lw projection or plain sum over fields) and second[b] (sum over d): 16 lanes per sample each take
// every 16th term, then a 16-lane DPP sum
template <int RT>
__device__ __forceinline__ void stage_fs(const FwdArgs& p, const StageScratch sc, float* fs, int lane, int wave) {
  constexpr int D = 10;
  constexpr int ROWS = 16 * RT;
  const int F = p.F;
  const int flags = p.flags;
  const int Fp = r4(F);
  for (int g4 = wave; g4 * 4 < ROWS; g4 += kFW) {
    const int b = g4 * 4 + (lane >> 4);
    const int qd = lane & 15;
    float first = 0.f, second = 0.f;
    for (int f0 = 0; f0 < F; f0 += 64) {
      float x[4], l[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int f = min(f0 + 16 * k + qd, F - 1);
        x[k] = sc.fo[b * Fp + f];
        l[k] = (flags & kFoLw) ? sc.lw[f] : 1.f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) first = f0 + 16 * k + qd < F ? fmaf(x[k], l[k], first) : first;
    }
    if (flags & kHasSecond)
      for (int d = qd; d < D; d += 16) second += sc.part2[b * D + d];  // the sample's column sums
    first = sum16(first);
    second = sum16(second);
    if (qd == 0) fs[b] = first + second;
  }
}

// one layer's K loop of one wave over its TPW output tiles (wt[j]: the tile's fragments of K step 0): PD weight
// fragment sets in a ring, each loaded PD - 1 steps ahead of its MFMAs (the L2 round trip); unrolled by PD so no set
// is copied.  mma(c, wq) fetches K step c's activation fragments and issues the step's MFMAs on the set wq.
template <int PD, int TPW, class Mma>
__device__ __forceinline__ void ring_k_loop(const u32x4* const (&wt)[TPW], int lane, int KC, Mma mma) {
  u32x4 wf[PD][TPW];
  auto load = [&](int c, u32x4(&wq)[TPW]) {
#pragma unroll
    for (int j = 0; j < TPW; ++j) wq[j] = (wt[j] + c * 64)[lane];  // a wave-uniform base, the lane as the offset
  };
#pragma unroll
  for (int p = 0; p < PD - 1; ++p)
    if (p < KC) load(p, wf[p]);
  int c = 0;
  for (; c + 2 * PD - 1 <= KC; c += PD) {  // steady state: every step's refill is in range
#pragma unroll
    for (int p = 0; p < PD; ++p) {
      load(c + p + PD - 1, wf[(p + PD - 1) % PD]);
      mma(c + p, wf[p]);
    }
  }
  for (; c < KC; c += PD) {  // the last 1 .. 2 PD - 2 steps (conditions wave-uniform)
#pragma unroll
    for (int p = 0; p < PD; ++p) {
      if (c + p < KC) {
        if (c + p + PD - 1 < KC) load(c + p + PD - 1, wf[(p + PD - 1) % PD]);
        mma(c + p, wf[p]);
      }
    }
  }
}

// the last layer's share of deep of one row and one 16-neuron tile (v: this lane's four outputs, fq: their fc
// weights), as layer_epilogue forms it, to *dst from the quarter's first 16 lanes; every lane takes part in the
// shuffles
__device__ __forceinline__ void last_layer_share(f32x4 v, f32x4 fq, int lv, float* dst) {
  float d = 0.f;
  d = fmaf(v[0], fq[0], d);
  d = fmaf(v[1], fq[1], d);
  d = fmaf(v[2], fq[2], d);
  d = fmaf(v[3], fq[3], d);
  d += __shfl_xor(d, 16);
  d += __shfl_xor(d, 32);
  if (lv < 16) *dst = d;
}

// logit[b] = (first_second[b] + the shares [ROWS][NT] in tile order) + bias, as bf16_combine_kernel
template <int ROWS>
__device__ __forceinline__ void stage_logits(const FwdArgs& p, const TileRef tr, const float* part, const float* fs,
                                             int NT, int tid) {
  if (tid < ROWS && tr.b0 + tid < p.batch) {
    const float* pp = part + tid * NT;
    float deep = pp[0];
    for (int t = 1; t < NT; ++t) deep += pp[t];
    tr.out[tr.b0 + tid] = (fs[tid] + deep) + p.bias[0];
  }
}

// the launch of one instantiation: the workgroups of `rows` rows each, the dynamic-LDS limit raised once per kernel
template <class Geo>
inline hipError_t launch_fused_kernel(void (*k)(const FwdArgs, const Geo), const FwdArgs& a, const Geo& g, int rows,
                                      int threads, size_t lds, hipStream_t s) {
  const hipError_t e = ensure_lds_limit(reinterpret_cast<const void*>(k), lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k, dim3(fwd_grid(a, rows)), dim3(threads), lds, s, a, g);
  return hipGetLastError();
}

}  // namespace dfwfm
