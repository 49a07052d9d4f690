// conv3x3 (pad 1) forward / dgrad / wgrad for a whole meta-batch in one launch, per-task weights.
//
// Replaces the implicit ATen conv2d forward / backward / double-backward launches behind ConvBlock.conv
// (reference core_functions/vision_models.py:177-185,189) for every task of the meta-batch at once.
//
// Design (gfx950): implicit GEMM on the exact-fp32 matrix pipe, v_mfma_f32_32x32x2_f32 (bitwise an fmaf chain, so the
// fp32 parity budget is untouched).  One wave owns a 32-pixel x 32-channel output tile (M = pixels of the task in
// (n,y,x) raster order, N = output channels): 32 filters -- the reference's hidden size -- is exactly one MFMA tile.
// K = 9 taps x Ci; the K order is free, so lane half h = lane>>5 takes input channels [16h,16h+16) of each 32-channel
// chunk: one lane's A operands for 16 consecutive MFMAs are 16 contiguous NHWC floats (4 x 16-B loads), no shuffles.
// Per-task weights are staged once per workgroup into LDS as [term][tap][ci][32] (B operand reads are conflict-free,
// 32 consecutive dwords per lane half) and re-used for every pixel tile the workgroup walks.
// "terms": the tangent (R-operator) passes need conv(x,Wd)+conv(xd,W) / dgrad(Rdz,W)+dgrad(dz,Wd); both products
// accumulate into the same MFMA accumulators in one launch.
// Epilogues: per-(task,channel) fp64 partial sums for batch-stat BN (sum z, sum z^2) or its tangent (sum zd, sum zh*zd),
// reduced wave -> workgroup in LDS and written as one deterministic partial per workgroup (no atomics).
// Split-bf16 operand form (template flag BF of the stride-1 kernel, 32 filters and one-term 64 filters; default, see
// mi_conv_set_split_bf16 and bf16_split.h): every fp32 operand as three exact bf16 planes, six v_mfma_f32_32x32x16_bf16 products per
// K = 16, fp32 accumulation -- fp32-equivalent results on the 16x faster pipe.  Tiles of 30 output pixels (lanes 0 / 31 are halo lanes), a
// displaced image row fetched once and shifted across lanes for the horizontal taps, splits and shifts placed between the MFMAs.
#include "mi_common.h"
#include "kernels.h"
#include "bf16_split.h"
#include "fold.h"
#include <type_traits>

// Ablation build (timing / energy experiment, wrong results, not shipped): -DMI_CONV_ABLATE_LOW compiles out the three products of a K
// step that a two-plane operand form would not have (DESIGN.md 8c lead 5); build to another file name and select it with MI_MAML_LIB.
#ifdef MI_CONV_ABLATE_LOW
#define MI_LOW_PRODUCT(X)
#else
#define MI_LOW_PRODUCT(X) X
#endif
// Ablation build (timing experiment, wrong results, not shipped): -DMI_CONV_ABLATE_ROW drops the loads, splits and lane shifts of every
// third displaced row of a tile (the operands of the row before are used again): what a tile of two output rows that fetches four input
// rows for them would save at best.
#ifdef MI_CONV_ABLATE_ROW
#define MI_ROW_KEPT(i) (hg_ddy(i) != 1)
#else
#define MI_ROW_KEPT(i) true
#endif
#define EPI_NONE 0
#define EPI_STATS 1
#define EPI_TSTATS 2
#define EPI_BRED 3     // block-1 BatchNorm-backward sums in the epilogue of block 2's dgrad (kernels.h, ConvArgs::bp ...)

// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stats_block_reduce(double s, double q, double* ldsd, int lane, int wave, int nwaves,
                                                   double* partial_task, int co_total, int cbase, const FinArgs& fin, int task,
                                                   int bx = -1) {
  double* partial_blk = partial_task + (size_t)(bx < 0 ? (int)blockIdx.x : bx) * 2 * co_total;
  // lanes l and l^32 hold the same channel
  s += __shfl_xor(s, 32, 64);
  q += __shfl_xor(q, 32, 64);
  __syncthreads();  // weights in LDS are dead from here on
  if (lane < 32) {
    ldsd[(wave * 2 + 0) * 32 + lane] = s;
    ldsd[(wave * 2 + 1) * 32 + lane] = q;
  }
  __syncthreads();
  if (wave == 0 && lane < 32) {
    double ts = 0.0, tq = 0.0;
    for (int w = 0; w < nwaves; ++w) {
      ts += ldsd[(w * 2 + 0) * 32 + lane];
      tq += ldsd[(w * 2 + 1) * 32 + lane];
    }
    mi_partial_store(partial_blk + cbase + lane, ts, fin);
    mi_partial_store(partial_blk + co_total + cbase + lane, tq, fin);
  }
  mi_finalize_last(fin, partial_task, gridDim.x, co_total, task, gridDim.x * gridDim.z, ldsd);
}

template <int EPI>
__device__ __forceinline__ void conv_epilogue(const floatx16& acc, int tile, int lane, int mpix, int co_total, int cbase,
                                              float* __restrict__ out_t, const float* zpre, float mu_c, float r_c, double& s,
                                              double& q) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = (r & 3) + 8 * (r >> 2) + 4 * h;
    const int pix = tile * 32 + m;
    if (pix < mpix) {
      const size_t o = (size_t)pix * co_total + cbase + j;
      const float v = acc[r];
      out_t[o] = v;
      if (EPI == EPI_STATS) {
        const double dv = (double)v;
        s += dv;
        q = fma(dv, dv, q);
      } else if (EPI == EPI_TSTATS) {
        const float zh = bn_zh(zpre[r], mu_c, r_c);      // z was prefetched at the top of the tile, under the MFMAs
        s += (double)v;
        q = fma((double)zh, (double)v, q);
      }
    }
  }
}

// z values of this lane's 16 output positions (tangent-stat epilogue), issued before the MFMA loop of the tile
__device__ __forceinline__ void conv_prefetch_z(float* zpre, const float* __restrict__ z_t, int tile, int lane, int mpix,
                                                int co_total, int cbase) {
  const int j = lane & 31, h = lane >> 5;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int pix = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    zpre[r] = *(pix < mpix ? z_t + ((size_t)pix * co_total + cbase + j) : mi_zero_word);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Generic conv: CI multiple of 32 (template), CO multiple of 32 (grid.z tiles).
// MODE 0: forward   out[o] = sum_tap in[o*S + d - 1] * W[tap]            weights [9][CI][CO]
// MODE 1: dgrad     out[i] = sum_tap in[(i + 1 - d)/S] * W[tap]^T        weights [9][CO_op][CI_op] (the forward layout)
// waves per workgroup: the 2-term variants stage 2 x 36 KB of weights, so 8 waves share one copy (2 workgroups = 4 waves/SIMD)
#ifndef MI_F16_WIDE
// The fp16 form needs two thirds of the bf16 form's LDS and fewer registers, so eight-wave workgroups at four waves per SIMD fit
// (-DMI_F16_WIDE=1).  Measured on one box, two repeats each: 15.69 / 15.65 ms per cfg2 iteration wide against 15.51 / 15.54 with the
// bf16 form's shapes (two waves per SIMD) -- occupancy is not what these kernels wait for.  Default: the bf16 form's shapes.
#define MI_F16_WIDE 0
#endif
template <int CI, int NTERMS, bool BF = false, bool F16 = false> struct ConvWaves {
  // (split-bf16 form at 64 filters: 108 KB of weight planes per workgroup -> one workgroup per CU, so eight waves share it)
  // (fp16 form with MI_F16_WIDE: always eight -- two workgroups per CU share two staged weight copies among 16 waves, four per SIMD)
  static constexpr int value = ((F16 && MI_F16_WIDE) || (NTERMS == 2 && CI == 32) || (BF && CI == 64)) ? 8 : 4;
};
// fp16 form with MI_F16_WIDE: the variants that fit 128 registers are built for four waves per SIMD (the tangent-statistics epilogue does not)
template <int EPI, bool F16> struct ConvWavesPerSimd { static constexpr int value = (F16 && MI_F16_WIDE && EPI != 2 /* EPI_TSTATS */) ? 4 : 1; };
// Measured (rocprofv3 SQ counters + hipOccupancy): the 2-term EPI_TSTATS variant takes 178 VGPRs, so one 8-wave workgroup is
// resident per CU (1.8 waves/SIMD) while the 2-term dgrad (108 VGPRs, two workgroups, 2.9 waves/SIMD) reaches the same 74 % MFMA
// busy fraction: occupancy is not the limiter.  Forcing <= 128 VGPRs (__launch_bounds__(512, 4)) spills 17 dwords into the
// main loop and is 13 % slower.

template <int CI, int NTERMS, int EPI, int MODE, int STRIDE>
__global__ __launch_bounds__((ConvWaves<CI, NTERMS>::value * 64)) void conv3x3_mfma_kernel(ConvArgs a) {
  constexpr int NW = ConvWaves<CI, NTERMS>::value, NT = NW * 64;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  const int task = blockIdx.y, ct = blockIdx.z;
  const int H = a.g.h, W = a.g.w, HO = a.g.ho, WO = a.g.wo, CO = a.g.co;
  const int cbase = ct * 32;

  // ---- stage this task's weights: lds[((term*9+tap)*CI + k)*32 + nl], 16 bytes per load.  Forward: a weight row's 32 filters
  // are contiguous in [tap][ci][co], so a quad of nl is one float4 copy.  dgrad: the quad runs along k (contiguous in the forward
  // layout [tap][co][ci]) and is scattered into four LDS rows.
  constexpr int NQ = NTERMS * 9 * CI * 32 / 4;
#pragma unroll 3
  for (int qd = tid; qd < NQ; qd += NT) {
    if (MODE == 0) {
      const int nl4 = (qd & 7) * 4;
      const int row = qd >> 3;                 // (term*9 + tap)*CI + k
      const int k = row % CI, tt = row / CI;
      const int term = tt / 9, tap = tt - term * 9;
      const float* wsrc = a.wt[term] + (size_t)task * a.wstride;
      const floatx4 v = *reinterpret_cast<const floatx4*>(wsrc + ((size_t)tap * CI + k) * CO + cbase + nl4);
      *reinterpret_cast<floatx4*>(lds + row * 32 + nl4) = v;
    } else {
      constexpr int KQ = CI / 4;               // quads along k
      const int k4 = (qd % KQ) * 4;
      const int rest = qd / KQ;                // (term*9 + tap)*32 + nl
      const int nl = rest & 31, tt = rest >> 5;
      const int term = tt / 9, tap = tt - term * 9;
      const float* wsrc = a.wt[term] + (size_t)task * a.wstride;
      const floatx4 v = *reinterpret_cast<const floatx4*>(wsrc + ((size_t)tap * CO + cbase + nl) * CI + k4);
      float* dst = lds + ((size_t)tt * CI + k4) * 32 + nl;
      dst[0] = v[0]; dst[32] = v[1]; dst[64] = v[2]; dst[96] = v[3];
    }
  }
  __syncthreads();

  const int mpix = a.mpix;
  const size_t in_task = (size_t)a.g.n * H * W * CI;
  const size_t out_task = (size_t)mpix * CO;
  float* out_t = a.out + (size_t)task * out_task;
  const float* z_t = (EPI == EPI_TSTATS) ? a.z + (size_t)task * out_task : nullptr;
  float mu_c = 0.f, r_c = 0.f;
  if (EPI == EPI_TSTATS) {
    mu_c = a.mu[(size_t)task * CO + cbase + j];
    r_c = a.rstd[(size_t)task * CO + cbase + j];
  }
  double s = 0.0, q = 0.0;

  // Main loop: explicit software pipeline over the K steps (term, tap, 32-channel chunk).  Each step's A operand is 16
  // contiguous NHWC floats of this lane's (shifted) pixel = 4 x 16-B loads, issued DEPTH steps ahead of the 16 MFMAs that
  // consume them; padding lanes read mi_zero_word through an address select (no predicated loads, no post-load selects).
  // sched_barriers pin the order so the compiler neither hoists every load to the top (register blow-up) nor sinks them.
  constexpr int NCC = CI / 32, NSTEP = NTERMS * 9 * NCC, DEPTH = 2, RING = DEPTH + 1;
  // (16-B operands use global loads with an address select here; the stride-1 kernel below uses raw buffer loads.)
  const float* in_base[NTERMS];
#pragma unroll
  for (int term = 0; term < NTERMS; ++term) in_base[term] = a.in[term] + (size_t)task * in_task + h * 16;

  // tiles are interleaved over the workgroup's waves (wave w takes tiles base + w, base + w + NW, ...): at any time the waves
  // work on adjacent image rows and share the 3x3 halo in L1/L2 instead of each sweeping its own far-apart chunk.
  const int tile_base = blockIdx.x * NW * a.tiles_per_wave;
  const int tile_end = min(tile_base + NW * a.tiles_per_wave, a.ntiles);
  for (int tile = tile_base + wave; tile < tile_end; tile += NW) {
    const int pix = tile * 32 + j;
    const bool valid = pix < mpix;
    const int n = pix / (HO * WO);
    const int rem = pix - n * (HO * WO);
    const int oy = rem / WO, ox = rem - oy * WO;
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    float zpre[16];
    if (EPI == EPI_TSTATS) conv_prefetch_z(zpre, z_t, tile, lane, mpix, CO, cbase);
    float4 ring[RING][4];
    auto issue = [&](int step, float4* dst) {
      const int cc = step % NCC, tt = step / NCC, tap = tt % 9, term = tt / 9;
      const int dy = tap / 3, dx = tap % 3;
      int iy, ix;
      bool inb = valid;
      if (MODE == 0) {
        iy = oy * STRIDE + dy - 1;
        ix = ox * STRIDE + dx - 1;
      } else {
        iy = oy + 1 - dy;
        ix = ox + 1 - dx;
        if (STRIDE == 2) {
          inb = inb && ((iy & 1) == 0) && ((ix & 1) == 0);
          iy >>= 1;
          ix >>= 1;
        }
      }
      inb = inb && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
      const float* src = inb ? in_base[term] + (((n * H + iy) * W + ix) * CI + cc * 32) : mi_zero_word;
      const float4* s4 = reinterpret_cast<const float4*>(src);
      dst[0] = s4[0]; dst[1] = s4[1]; dst[2] = s4[2]; dst[3] = s4[3];
    };
#pragma unroll
    for (int st = 0; st < DEPTH && st < NSTEP; ++st) issue(st, ring[st % RING]);
#pragma unroll
    for (int step = 0; step < NSTEP; ++step) {
      if (step + DEPTH < NSTEP) issue(step + DEPTH, ring[(step + DEPTH) % RING]);
      __builtin_amdgcn_sched_barrier(0);
      const int cc = step % NCC, tt = step / NCC;           // tt = term*9 + tap
      const float4* av = ring[step % RING];
      const float* bl = lds + ((size_t)(tt * CI + cc * 32 + h * 16)) * 32 + j;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v].x, bl[(4 * v + 0) * 32], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v].y, bl[(4 * v + 1) * 32], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v].z, bl[(4 * v + 2) * 32], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v].w, bl[(4 * v + 3) * 32], acc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    conv_epilogue<EPI>(acc, tile, lane, mpix, CO, cbase, out_t, zpre, mu_c, r_c, s, q);
  }
  if (EPI != EPI_NONE) {
    double* pb = a.partial + (size_t)task * gridDim.x * 2 * CO;
    stats_block_reduce(s, q, reinterpret_cast<double*>(lds), lane, wave, NW, pb, CO, cbase, a.fin, task);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-1 variant of the generic conv (every pooling net: blocks >= 2 forward, dgrad and their two-term tangent versions).
// Input and output have the same spatial size, so an output pixel's linear index IS the linear index of the input pixel under
// the kernel centre and tap (ddy, ddx) sits at the constant displacement (ddy*W + ddx)*CI floats: per tile a lane computes ONE
// byte offset, per K step it adds a wave-uniform displacement and substitutes an out-of-range offset for padding lanes.  All
// operands come through raw buffer loads (16 B each, immediate offsets for the four quarters of a 64-B half row): the hardware
// range check returns zeros for padding, so there are no predicated loads, no 64-bit address arithmetic and no integer
// multiplies in the main loop.  The epilogue stores through a buffer descriptor as well (rows past the end of the task are
// dropped by the range check) and the statistics need no validity test: a pixel past the end has all-zero operands, hence
// acc == 0 exactly.  Requires co == CI (hidden -> hidden blocks) and fewer than 2^24 pixels per task.
// x / d and x % d for x < 2^24 with the reciprocal of d in fp32: the fp32 quotient is off by at most one
__device__ __forceinline__ void divmod24(unsigned x, unsigned d, float rd, unsigned& q, unsigned& r) {
  q = (unsigned)((float)x * rd);
  int rr = (int)x - (int)__umul24(q, d);
  if (rr < 0) { --q; rr += (int)d; }
  if (rr >= (int)d) { ++q; rr -= (int)d; }
  r = (unsigned)rr;
}

// ---- split-bf16 operands (BF variants of the stride-1 kernel): bf16_split.h
// A store the compiler's wait-count bookkeeping does not see.  gfx9 counts loads and stores in ONE counter and lets them complete out of
// order with respect to each other, so with a visible store pending hipcc turns every wait for an operand load into vmcnt(0) -- which also
// drains the prefetched loads of the next two half-groups, at every tile boundary.  Hidden, the stores only ever make a counted wait
// longer (loads still complete in issue order among themselves), never shorter; nothing in the kernel reads what they write.
__device__ __forceinline__ void buf_st_untracked(mi_u32x4 rsrc, unsigned off, float v) {
  asm volatile("buffer_store_dword %0, %1, %2, 0 offen" : : "v"(v), "v"(off), "s"(rsrc) : "memory");
}
struct Bf16Planes { unsigned h[4], m[4], l[4]; };              // 8 values: three bf16x8 operands
template <int P>
__device__ __forceinline__ void bf16_split_pair(const floatx4& x, Bf16Planes& p) {       // values 2P, 2P + 1 of the eight (x = their float4)
#ifdef MI_CONV_ABLATE_SPLIT
  // Ablation build (timing / energy experiment, wrong results, not shipped): the loaded bits stand in for the three planes -- what operands
  // that arrive already split (written as planes by their producer) would save at most, before their 50 % larger loads.
  p.h[P] = __builtin_bit_cast(unsigned, x[(P & 1) * 2]); p.m[P] = __builtin_bit_cast(unsigned, x[(P & 1) * 2 + 1]); p.l[P] = p.h[P] ^ p.m[P];
#else
  bf16_split2(floatx2{x[(P & 1) * 2], x[(P & 1) * 2 + 1]}, p.h[P], p.m[P], p.l[P]);
#endif
  asm volatile("" : "+v"(p.h[P]), "+v"(p.m[P]), "+v"(p.l[P]));     // computed HERE (instruction selection otherwise sinks the split to its use)
}
__device__ __forceinline__ void bf16_split8(const floatx4& x0, const floatx4& x1, Bf16Planes& p) {
  bf16_split_pair<0>(x0, p); bf16_split_pair<1>(x0, p); bf16_split_pair<2>(x1, p); bf16_split_pair<3>(x1, p);
}

// debug aid: shader-clock stamps of workgroup (0, 0, 0)'s wave 0 (mi_debug_conv_stamps; null in production)
__device__ unsigned long long* g_conv_stamps = nullptr;
#ifndef MI_CONV_STAMP_TILES
#define MI_CONV_STAMP_TILES 0
#endif
#define CV_STAMP(k) do { if (cstamp && tid == 0) cstamp[k] = __builtin_amdgcn_s_memtime(); } while (0)

// F16 (with BF): the two-plane fp16 operand form (bf16_split.h) -- same tiles, loads and lane shifts, two planes and three products
// per K step, the scales from ConvArgs::amax (activations, per task) and from the staged weights themselves (per workgroup).
template <int CI, int NTERMS, int EPI, int MODE, bool BF = false, bool F16 = false>
__global__ __launch_bounds__((ConvWaves<CI, NTERMS, BF, F16>::value * 64), (ConvWavesPerSimd<EPI, F16>::value)) void conv3x3_s1_mfma_kernel(ConvArgs a) {
  static_assert(BF || !F16, "the fp16 form is a variant of the split kernel");
  constexpr int NW = ConvWaves<CI, NTERMS, BF, F16>::value, NT = NW * 64, CO = CI;
  constexpr int NPL = F16 ? 2 : 3;                              // operand planes
  constexpr int NCC = CI / 32, NSTEP = NTERMS * 9 * NCC;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 31, h = lane >> 5;
  // XCD-aware placement: workgroups are dealt to the 8 XCDs round-robin in linear launch order, so the 16..32 workgroups of one task
  // (adjacent bands of the same images, the same staged weights) would land on all eight L2s.  Re-deal the linear index so that
  // XCD k works through a contiguous run of (task, band) pairs: a task's halo rows and weights are fetched into ONE L2.
  int bx = blockIdx.x, task = blockIdx.y, ct = blockIdx.z;
  {
    const unsigned total = gridDim.x * gridDim.y * gridDim.z;
    if ((total & 7u) == 0u) {
      const unsigned lin = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      const unsigned nl = (lin & 7u) * (total >> 3) + (lin >> 3);
      // (the output-channel tiles of one band are neighbours in the run: they read the same input rows at the same time through one L2)
      ct = (int)(nl % gridDim.z);
      bx = (int)((nl / gridDim.z) % gridDim.x);
      task = (int)(nl / (gridDim.z * gridDim.x));
    }
  }
  const int H = a.g.h, W = a.g.w;
  const int cbase = ct * 32;
  unsigned long long* cstamp = (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0) ? g_conv_stamps : nullptr;
  CV_STAMP(0);

  // ---- stage this task's weights (same layout as the generic kernel): lds[((term*9+tap)*CI + k)*32 + nl]
  // BF: three bf16 planes per weight, in MFMA operand order: 16-B unit ((step*2 + kb)*3 + plane)*64 + lane holds, for lane (h, j),
  // the 8 values k = cc*32 + h*16 + kb*8 + 0..7 of output channel cbase + j  (step = (term*9 + tap)*NCC + cc)
  constexpr int NQ = BF ? 0 : NTERMS * 9 * CI * 32 / 4;
  float f16_sa[NTERMS], f16_sw[NTERMS], f16_inv = 1.f;           // F16: scales of the activations / the weights per term, 1 / (their product)
#pragma unroll
  for (int t = 0; t < NTERMS; ++t) { f16_sa[t] = 1.f; f16_sw[t] = 1.f; }
  unsigned f16_amax[NTERMS];                                     // F16: the activations' largest-magnitude cells, fetched before anything else
#pragma unroll
  for (int t = 0; t < NTERMS; ++t) f16_amax[t] = 0u;
  if constexpr (F16) {
#pragma unroll
    for (int t = 0; t < NTERMS; ++t) f16_amax[t] = mi_cell_fetch(a.amax[t], task);
  }
  if constexpr (BF) {
    mi_u32x4* l4 = reinterpret_cast<mi_u32x4*>(lds);
    constexpr int NIT = NSTEP * 2 * 64, IPT = (NIT + NT - 1) / NT;   // items (8 weights of one output channel) per thread
    // all of a thread's loads first, then the splits: one memory latency per workgroup instead of one per item
    floatx4 w0[IPT], w1[IPT];
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
      const int it = tid + q * NT;
      const int ln = it & 63, grp = it >> 6;
      const int jj = ln & 31, hb = ln >> 5, kb = grp & 1, stp = grp >> 1;
      const int cc = stp % NCC, tt = stp / NCC, term = tt / 9, tap = tt - term * 9;
      const int k0 = cc * 32 + hb * 16 + kb * 8;
      const bool live = it < NIT;
      const float* wsrc = a.wt[live ? term : 0] + (size_t)task * a.wstride;
      if (MODE == 0) {
        const float* src = wsrc + ((size_t)(live ? tap : 0) * CI + k0) * CO + cbase + jj;
#pragma unroll
        for (int i = 0; i < 4; ++i) { w0[q][i] = src[(size_t)i * CO]; w1[q][i] = src[(size_t)(i + 4) * CO]; }
      } else {
        const float* src = wsrc + ((size_t)(live ? tap : 0) * CO + cbase + jj) * CI + k0;
        w0[q] = *reinterpret_cast<const floatx4*>(src);
        w1[q] = *reinterpret_cast<const floatx4*>(src + 4);
      }
    }
    if constexpr (F16) {
      // the weights' scale: the largest magnitude among the weights THIS workgroup stages (all taps and input channels of its 32
      // filters: every K sum of its accumulators runs over exactly these), per term -- threads, then lanes, then waves through LDS
      float mx[NTERMS];
#pragma unroll
      for (int t = 0; t < NTERMS; ++t) mx[t] = 0.f;
#pragma unroll
      for (int q = 0; q < IPT; ++q) {
        const int it = tid + q * NT;
        float m = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) m = fmaxf(m, fmaxf(fabsf(w0[q][i]), fabsf(w1[q][i])));
        if (it >= NIT) m = 0.f;
        if (NTERMS == 1) mx[0] = fmaxf(mx[0], m);
        else { const bool t1 = (it >> 7) / NCC >= 9; mx[0] = fmaxf(mx[0], t1 ? 0.f : m); mx[NTERMS - 1] = fmaxf(mx[NTERMS - 1], t1 ? m : 0.f); }
      }
      float* red = lds + (size_t)NSTEP * 2 * NPL * 64 * 4;       // behind the planes (the launcher adds 64 B)
#pragma unroll
      for (int t = 0; t < NTERMS; ++t) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) mx[t] = fmaxf(mx[t], __shfl_xor(mx[t], o, 64));
        if (lane == 0) red[wave * NTERMS + t] = mx[t];
      }
      __syncthreads();
      int kk[2][2] = {{0, 0}, {0, 0}};                           // [term][0 = activations, 1 = weights]
#pragma unroll
      for (int t = 0; t < NTERMS; ++t) {
        float m = red[t];
#pragma unroll
        for (int w = 1; w < NW; ++w) m = fmaxf(m, red[w * NTERMS + t]);
        kk[t][1] = f16_scale_exp(__float_as_uint(m));
        kk[t][0] = f16_scale_exp(mi_cell_fold(f16_amax[t]));
      }
      if (NTERMS == 2) f16_common_scale(kk);
#pragma unroll
      for (int t = 0; t < NTERMS; ++t) {
        f16_sa[t] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(f16_pow2(kk[t][0]))));
        f16_sw[t] = f16_pow2(kk[t][1]);
      }
      f16_inv = f16_pow2(-(kk[0][0] + kk[0][1]));
    }
#pragma unroll
    for (int q = 0; q < IPT; ++q) {
      const int it = tid + q * NT;
      if (it < NIT) {
        const int ln = it & 63, grp = it >> 6;
        if constexpr (F16) {
          const float sw = (NTERMS == 2 && (grp >> 1) / NCC >= 9) ? f16_sw[NTERMS - 1] : f16_sw[0];
          unsigned ph[4], pl[4];
          f16_split2_v(floatx2{w0[q][0], w0[q][1]}, sw, ph[0], pl[0]);
          f16_split2_v(floatx2{w0[q][2], w0[q][3]}, sw, ph[1], pl[1]);
          f16_split2_v(floatx2{w1[q][0], w1[q][1]}, sw, ph[2], pl[2]);
          f16_split2_v(floatx2{w1[q][2], w1[q][3]}, sw, ph[3], pl[3]);
          l4[(grp * 2 + 0) * 64 + ln] = mi_u32x4{ph[0], ph[1], ph[2], ph[3]};
          l4[(grp * 2 + 1) * 64 + ln] = mi_u32x4{pl[0], pl[1], pl[2], pl[3]};
        } else {
          Bf16Planes pw;
          bf16_split8(w0[q], w1[q], pw);
          l4[(grp * 3 + 0) * 64 + ln] = mi_u32x4{pw.h[0], pw.h[1], pw.h[2], pw.h[3]};
          l4[(grp * 3 + 1) * 64 + ln] = mi_u32x4{pw.m[0], pw.m[1], pw.m[2], pw.m[3]};
          l4[(grp * 3 + 2) * 64 + ln] = mi_u32x4{pw.l[0], pw.l[1], pw.l[2], pw.l[3]};
        }
      }
    }
  }
#pragma unroll 3
  for (int qd = tid; qd < NQ; qd += NT) {
    if (MODE == 0) {
      const int nl4 = (qd & 7) * 4;
      const int row = qd >> 3;
      const int k = row % CI, tt = row / CI;
      const int term = tt / 9, tap = tt - term * 9;
      const float* wsrc = a.wt[term] + (size_t)task * a.wstride;
      const floatx4 v = *reinterpret_cast<const floatx4*>(wsrc + ((size_t)tap * CI + k) * CO + cbase + nl4);
      *reinterpret_cast<floatx4*>(lds + row * 32 + nl4) = v;
    } else {
      constexpr int KQ = CI / 4;
      const int k4 = (qd % KQ) * 4;
      const int rest = qd / KQ;
      const int nl = rest & 31, tt = rest >> 5;
      const int term = tt / 9, tap = tt - term * 9;
      const float* wsrc = a.wt[term] + (size_t)task * a.wstride;
      const floatx4 v = *reinterpret_cast<const floatx4*>(wsrc + ((size_t)tap * CO + cbase + nl) * CI + k4);
      float* dst = lds + ((size_t)tt * CI + k4) * 32 + nl;
      dst[0] = v[0]; dst[32] = v[1]; dst[64] = v[2]; dst[96] = v[3];
    }
  }
  // (no barrier yet: the first operand loads go out before the wait for the staged weights, see below)

  const int mpix = a.mpix;
  const unsigned hw = (unsigned)(H * W);
  const float rhw = 1.0f / (float)hw, rw = 1.0f / (float)W;
  const size_t t_elems = (size_t)mpix * CI;                 // input and output tensors of one task have the same size (co == CI)
  const unsigned t_bytes = (unsigned)(t_elems * 4);
  mi_rsrc rin[NTERMS];
#pragma unroll
  for (int term = 0; term < NTERMS; ++term)
    rin[term] = __builtin_amdgcn_make_buffer_rsrc((void*)(a.in[term] + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
  const mi_rsrc rout = __builtin_amdgcn_make_buffer_rsrc((void*)(a.out + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
  const unsigned long long out_addr = (unsigned long long)(a.out + (size_t)task * t_elems);
  const mi_u32x4 rout_raw = {(unsigned)out_addr, (unsigned)(out_addr >> 32) & 0xffffu, t_bytes, 0x00020000u};   // = rout, as plain words
  mi_rsrc rz = rout;
  float mu_c = 0.f, r_c = 0.f;
  if (EPI == EPI_TSTATS) {
    rz = __builtin_amdgcn_make_buffer_rsrc((void*)(a.z + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
    mu_c = a.mu[(size_t)task * CO + cbase + j];
    r_c = a.rstd[(size_t)task * CO + cbase + j];
  }
  mi_rsrc rbp = rout, rbzh = rout, rbzhd = rout, rbdp = rout;
  // (EPI_BRED) "ReLU on" from the block's argmax byte where it has one (block 1: a quarter of p's bytes), else from p itself
  const bool bred_arg = EPI == EPI_BRED && a.barg != nullptr;
  if (EPI == EPI_BRED) {
    if (bred_arg) rbp = __builtin_amdgcn_make_buffer_rsrc((void*)(a.barg + (size_t)task * t_elems), 0, (unsigned)t_elems, 0x00020000);
    else rbp = __builtin_amdgcn_make_buffer_rsrc((void*)(a.bp + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
    rbzh = __builtin_amdgcn_make_buffer_rsrc((void*)(a.bzh + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
    if (NTERMS == 2) {
      rbzhd = __builtin_amdgcn_make_buffer_rsrc((void*)(a.bzhd + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
      rbdp = __builtin_amdgcn_make_buffer_rsrc((void*)(a.bdp + (size_t)task * t_elems), 0, t_bytes, 0x00020000);
    }
  }
  double s = 0.0, q = 0.0;
  // byte displacement of every tap (wave-uniform): forward reads in[o + d - 1], dgrad reads in[i + 1 - d]
  const int wci = W * CI * 4;
  const unsigned lane_in = (unsigned)(h * 64);
  const unsigned lane_out = (unsigned)(((4 * h) * CO + cbase + j) * 4);

  constexpr int DEPTH = 2, RING = DEPTH + 1;
  static_assert(NSTEP % RING == 0, "the operand ring must be in phase at every tile boundary");
  const int tile_base = bx * NW * a.tiles_per_wave;
  const int tile_end = min(tile_base + NW * a.tiles_per_wave, a.ntiles);
  // The operand pipeline runs ACROSS tiles: the last DEPTH steps of a tile already issue the first loads of the wave's next
  // tile, and the very first loads are issued before the barrier that ends the weight staging -- a wave never drains its loads at a
  // tile boundary (matters most where a wave has few tiles: blocks 3 and 4, few-image launches).
#ifndef MI_CONV_XTILE
#define MI_CONV_XTILE 1
#endif
  // BF: a tile is 30 output pixels; lanes j = 0 / 31 carry the pixel before / behind them -- operands for their neighbours' horizontal
  // taps, their own accumulator rows are dropped -- so no tap needs anything from outside the wave (7 % more MFMAs instead of an
  // "edge" load, its split and a merge per shifted register: half the vector instructions per row).
  constexpr int TP = BF ? 30 : 32, PO = BF ? 1 : 0;
  struct TileSt { unsigned base; bool rowok[3], colok[3]; unsigned keep_m, keep_p, offc[3]; };
  auto decode = [&](int tl) {
    TileSt t;
    const unsigned pix = (unsigned)(tl * TP + j - PO);              // tile 0, lane 0 of the BF form: "-1" wraps to an invalid pixel
    unsigned nimg, rem, oy, ox;
    divmod24(pix, hw, rhw, nimg, rem);
    divmod24(rem, (unsigned)W, rw, oy, ox);
    const bool valid = tl < tile_end && pix < (unsigned)mpix;       // past the wave's last tile: every load reads out of range (zeros)
    // row / column validity of the three vertical and horizontal displacements (index 0, 1, 2 <-> -1, 0, +1)
    t.rowok[0] = valid && oy >= 1u; t.rowok[1] = valid; t.rowok[2] = valid && oy + 1u < (unsigned)H;
    t.colok[0] = ox >= 1u; t.colok[1] = true; t.colok[2] = ox + 1u < (unsigned)W;
    t.base = pix * (unsigned)(CI * 4) + lane_in;
    if constexpr (BF) {
      // operands of the horizontal displacements -1 / +1 are the centre operand one lane over (DPP wave shift), zero where the pixel sits
      // in the image's first / last column (as bit masks fused into the shift: a v_cndmask_b32 costs four plain VALU instructions here,
      // tools/valu_rate_probe.hip); opaque, so that the optimiser cannot turn the AND back into a select
      t.keep_m = t.colok[0] ? 0xffffffffu : 0u;
      t.keep_p = t.colok[2] ? 0xffffffffu : 0u;
      asm volatile("" : "+v"(t.keep_m), "+v"(t.keep_p));
      // byte offsets of the centre loads of the three displaced rows (out of range where the row is padding)
#pragma unroll
      for (int d = 0; d < 3; ++d) t.offc[d] = t.rowok[d] ? t.base + (unsigned)((d - 1) * wci) : MI_OOB;
    }
    return t;
  };
  auto issue = [&](const TileSt& t, int step, floatx4* dst) {
    const int cc = step % NCC, tt = step / NCC, tap = tt % 9, term = tt / 9;
    const int ddy = (MODE == 0) ? tap / 3 - 1 : 1 - tap / 3;
    const int ddx = (MODE == 0) ? tap % 3 - 1 : 1 - tap % 3;
    const bool ok = t.rowok[ddy + 1] && t.colok[ddx + 1];
    const unsigned off = ok ? t.base + (unsigned)(ddy * wci + ddx * CI * 4) : MI_OOB;
    dst[0] = buf_ld16(rin[term], off + cc * 128);
    dst[1] = buf_ld16(rin[term], off + cc * 128 + 16);
    dst[2] = buf_ld16(rin[term], off + cc * 128 + 32);
    dst[3] = buf_ld16(rin[term], off + cc * 128 + 48);
  };
  floatx4 ring[BF ? 1 : RING][4];
  int tile = tile_base + wave;
  TileSt cur = decode(tile);
  // ---- BF pipeline.  Half-group i of a tile = (term, row displacement, 32-channel chunk cc, k half kb): the lane's 8 values
  // k = cc*32 + 16h + 8kb + 0..7 of its pixel in the displaced row (2 x 16 B).  Three MFMA units per half-group (horizontal
  // displacement 0, -1, +1), six bf16 MFMAs each.  A row is fetched ONCE and shifted across lanes for the two other taps:
  // a third of the fp32 kernel's per-lane 16-B cache accesses (its L1 runs at 0.77 accesses per clock and CU, tools/conv_l1_probe.py).
#ifndef MI_F16_HRING
#define MI_F16_HRING 3
#endif
  // loads run two half-groups ahead of the split, three ahead of the MFMAs (fp16 form: a half-group is nine MFMAs instead of eighteen, but
  // a ring of six -- the same distance in time -- costs 24 registers, spills in the epilogues with sums, and measured 15.8 against 15.2 ms)
  constexpr int NH = NSTEP / 3 * 2, HRING = F16 ? MI_F16_HRING : 3;
  static_assert(NH % HRING == 0 && NH % 2 == 0, "raw ring and plane double buffer must be in phase at every tile boundary");
  floatx4 rawc[BF ? HRING : 1][2];
  auto hg_term = [](int i) { return i / (6 * NCC); };
  auto hg_ddy = [](int i) { return (i % (6 * NCC)) / (2 * NCC) - 1; };
  auto hg_cc = [](int i) { return (i / 2) % NCC; };
  auto hg_unit = [&](int i, int ddx) {                          // index of the unit's weights in LDS: ((term*9 + tap)*NCC + cc)*2 + kb
    const int ddy = hg_ddy(i);
    const int tap = (MODE == 0) ? (ddy + 1) * 3 + (ddx + 1) : (1 - ddy) * 3 + (1 - ddx);
    return ((hg_term(i) * 9 + tap) * NCC + hg_cc(i)) * 2 + (i & 1);
  };
  auto issue_hg = [&](const TileSt& t, int i) {
    const int ddy = hg_ddy(i), term = hg_term(i);
    const unsigned offc = t.offc[ddy + 1] + (unsigned)(hg_cc(i) * 128 + (i & 1) * 32);
    rawc[i % HRING][0] = buf_ld16(rin[term], offc);
    rawc[i % HRING][1] = buf_ld16(rin[term], offc + 16);
  };
  if constexpr (BF) {
#pragma unroll
    for (int i = 0; i < HRING; ++i) issue_hg(cur, i);
  } else {
#pragma unroll
    for (int st = 0; st < DEPTH; ++st) issue(cur, st, ring[st % RING]);
  }
  __syncthreads();                                            // weights staged (the first operand loads are already in flight)
  CV_STAMP(1);
  int ntile_done = 0;
  Bf16Planes pc[2], opm, opp;                                  // centre planes (double-buffered over half-groups), shifted operands
  mi_u32x4 pb[2][3];
  const mi_u32x4* l4 = reinterpret_cast<const mi_u32x4*>(lds) + lane;
  // F16: values 2P, 2P + 1 of a half-group's eight (x = their float4) into planes h / l of nc, scaled by the term's activation scale
#define MI_F16_PAIR(P, X, NC, S) { f16_split2(floatx2{(X)[((P) & 1) * 2], (X)[((P) & 1) * 2 + 1]}, S, NC.h[P], NC.l[P]); \
                                   asm volatile("" : "+v"(NC.h[P]), "+v"(NC.l[P])); }
  if constexpr (F16) {
    MI_F16_PAIR(0, rawc[0][0], pc[0], f16_sa[0]) MI_F16_PAIR(1, rawc[0][0], pc[0], f16_sa[0])
    MI_F16_PAIR(2, rawc[0][1], pc[0], f16_sa[0]) MI_F16_PAIR(3, rawc[0][1], pc[0], f16_sa[0])
    const int u0 = hg_unit(0, 0);
    pb[0][0] = l4[(u0 * 2 + 0) * 64]; pb[0][1] = l4[(u0 * 2 + 1) * 64];
  } else if constexpr (BF) {
    bf16_split8(rawc[0][0], rawc[0][1], pc[0]);
    const int u0 = hg_unit(0, 0);
    pb[0][0] = l4[(u0 * 3 + 0) * 64]; pb[0][1] = l4[(u0 * 3 + 1) * 64]; pb[0][2] = l4[(u0 * 3 + 2) * 64];
  }

  for (; tile < tile_end; tile += NW) {
    if (MI_CONV_STAMP_TILES && ntile_done == 1) CV_STAMP(2);   // a (flat) store inside the tile loop makes every operand wait of the first half-groups a vmcnt(0)
    ++ntile_done;
    const TileSt nxt = decode(tile + NW);
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;

    const unsigned obase = lane_out + (unsigned)(tile * TP - PO) * (unsigned)(CO * 4);      // (BF tile 0: "-1 pixel" wraps; row 0 is dropped anyway)
    float zpre[16];
    if (EPI == EPI_TSTATS) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned ro = (unsigned)(((r & 3) + 8 * ((r >> 2) & 1)) * CO * 4);
        zpre[r] = buf_ld(rz, obase + ((r >> 3) ? (unsigned)(16 * CO * 4) : 0u) + ro);
      }
    }
    if constexpr (F16) {
      // Half-group i: three units (horizontal displacement 0, -1, +1) of three products each; between them the lane shifts of this
      // half-group's planes (4 registers x 2 planes per displaced operand) and the split of the next half-group's eight values
#define MI_SHIFT(dst, P, R, CTRL, SEL) dst.P[R] = (unsigned)__builtin_amdgcn_mov_dpp((int)pc_.P[R], CTRL, 0xf, 0xf, true) & SEL;
#define MI_SHIFT4(dst, P, CTRL, SEL)                                                                     \
      { MI_SHIFT(dst, P, 0, CTRL, SEL) MI_SHIFT(dst, P, 1, CTRL, SEL) MI_SHIFT(dst, P, 2, CTRL, SEL) MI_SHIFT(dst, P, 3, CTRL, SEL) \
        asm volatile("" : "+v"(dst.P[0]), "+v"(dst.P[1]), "+v"(dst.P[2]), "+v"(dst.P[3])); }
#define MI_UNIT3(ca, cb, V0, V1, V2)                              \
      __builtin_amdgcn_sched_barrier(0);                          \
      acc = MI_F16_MFMA(ca.l, cb[0], acc);                        \
      __builtin_amdgcn_sched_barrier(0);                          \
      V0;                                                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      acc = MI_F16_MFMA(ca.h, cb[1], acc);                        \
      __builtin_amdgcn_sched_barrier(0);                          \
      V1;                                                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      acc = MI_F16_MFMA(ca.h, cb[0], acc);                        \
      __builtin_amdgcn_sched_barrier(0);                          \
      V2;                                                         \
      __builtin_amdgcn_sched_barrier(0);
#define MI_READB(dst, U) { dst[0] = l4[((U) * 2 + 0) * 64]; dst[1] = l4[((U) * 2 + 1) * 64]; }
#pragma unroll
      for (int i = 0; i < NH; ++i) {
        if (i + HRING < NH) issue_hg(cur, i + HRING); else issue_hg(nxt, i + HRING - NH);
        const Bf16Planes& pc_ = pc[i & 1];
        Bf16Planes& nc = pc[(i + 1) & 1];
        const floatx4* rc = rawc[(i + 1) % HRING];
        const float sn = f16_sa[hg_term((i + 1) % NH)];         // (compile-time index)
        const unsigned selm = cur.keep_m, selp = cur.keep_p;
        MI_READB(pb[(3 * i + 1) & 1], hg_unit(i, -1));
        MI_UNIT3(pc_, pb[(3 * i) & 1], MI_SHIFT4(opm, h, 0x138, selm), MI_SHIFT4(opm, l, 0x138, selm), MI_F16_PAIR(0, rc[0], nc, sn))
        MI_READB(pb[(3 * i + 2) & 1], hg_unit(i, 1));
        MI_UNIT3(opm, pb[(3 * i + 1) & 1], MI_SHIFT4(opp, h, 0x130, selp), MI_SHIFT4(opp, l, 0x130, selp), MI_F16_PAIR(1, rc[0], nc, sn))
        MI_READB(pb[(3 * i + 3) & 1], hg_unit((i + 1) % NH, 0));
        MI_UNIT3(opp, pb[(3 * i + 2) & 1], MI_F16_PAIR(2, rc[1], nc, sn), MI_F16_PAIR(3, rc[1], nc, sn), (void)0)
      }
#undef MI_READB
#undef MI_UNIT3
#undef MI_SHIFT4
#undef MI_SHIFT
    } else if constexpr (BF) {
      // shifted operand: lane <- the centre planes one lane over, zero in the image's first / last column (one v_and_b32_dpp per register)
#define MI_SHIFT(dst, P, R, CTRL, SEL) dst.P[R] = (unsigned)__builtin_amdgcn_mov_dpp((int)pc_.P[R], CTRL, 0xf, 0xf, true) & SEL;
#define MI_SHIFT6(dst, A0, A1, CTRL, SEL)                                                               \
      { MI_SHIFT(dst, A0, 0, CTRL, SEL) MI_SHIFT(dst, A0, 1, CTRL, SEL) MI_SHIFT(dst, A0, 2, CTRL, SEL) MI_SHIFT(dst, A0, 3, CTRL, SEL) \
        MI_SHIFT(dst, A1, 0, CTRL, SEL) MI_SHIFT(dst, A1, 1, CTRL, SEL)                                  \
        asm volatile("" : "+v"(dst.A0[0]), "+v"(dst.A0[1]), "+v"(dst.A0[2]), "+v"(dst.A0[3]), "+v"(dst.A1[0]), "+v"(dst.A1[1])); }
#define MI_SHIFT6B(dst, A1, A2, CTRL, SEL)                                                              \
      { MI_SHIFT(dst, A1, 2, CTRL, SEL) MI_SHIFT(dst, A1, 3, CTRL, SEL)                                  \
        MI_SHIFT(dst, A2, 0, CTRL, SEL) MI_SHIFT(dst, A2, 1, CTRL, SEL) MI_SHIFT(dst, A2, 2, CTRL, SEL) MI_SHIFT(dst, A2, 3, CTRL, SEL) \
        asm volatile("" : "+v"(dst.A1[2]), "+v"(dst.A1[3]), "+v"(dst.A2[0]), "+v"(dst.A2[1]), "+v"(dst.A2[2]), "+v"(dst.A2[3])); }
#define MI_UNIT(ca, cb, V1, V2, V3, V4)                           \
      __builtin_amdgcn_sched_barrier(0);                          \
      MI_LOW_PRODUCT(acc = MI_BF_MFMA(ca.l, cb[0], acc));         \
      __builtin_amdgcn_sched_barrier(0);                          \
      V1;                                                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      MI_LOW_PRODUCT(acc = MI_BF_MFMA(ca.h, cb[2], acc));         \
      __builtin_amdgcn_sched_barrier(0);                          \
      V2;                                                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      MI_LOW_PRODUCT(acc = MI_BF_MFMA(ca.m, cb[1], acc));         \
      __builtin_amdgcn_sched_barrier(0);                          \
      V3;                                                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      acc = MI_BF_MFMA(ca.m, cb[0], acc);                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      V4;                                                         \
      __builtin_amdgcn_sched_barrier(0);                          \
      acc = MI_BF_MFMA(ca.h, cb[1], acc);                         \
      acc = MI_BF_MFMA(ca.h, cb[0], acc);                         \
      __builtin_amdgcn_sched_barrier(0);
#define MI_READB(dst, U) { dst[0] = l4[((U) * 3 + 0) * 64]; dst[1] = l4[((U) * 3 + 1) * 64]; dst[2] = l4[((U) * 3 + 2) * 64]; }
      // Ablation build (timing / energy experiment, wrong results, not shipped): -DMI_CONV_ABLATE_LDS reads the weight planes of one unit
      // in three from LDS and uses them for the other two -- what sharing a weight read between two tiles of a wave could save at most.
#ifdef MI_CONV_ABLATE_LDS
#define MI_READB2(dst, U) { dst[0] = pb[0][0]; dst[1] = pb[0][1]; dst[2] = pb[0][2]; asm volatile("" : "+v"(dst[0]), "+v"(dst[1]), "+v"(dst[2])); }
#else
#define MI_READB2(dst, U) MI_READB(dst, U)
#endif
#pragma unroll
      for (int i = 0; i < NH; ++i) {
        // the loads of half-group i + 3 (the raw slot of half-group i was split during half-group i - 1)
        if (MI_ROW_KEPT((i + HRING) % NH)) { if (i + HRING < NH) issue_hg(cur, i + HRING); else issue_hg(nxt, i + HRING - NH); }
        const Bf16Planes& pc_ = pc[i & 1];
        Bf16Planes& nc = pc[(i + 1) & 1];
        const floatx4* rc = rawc[(i + 1) % HRING];
        const unsigned selm = cur.keep_m, selp = cur.keep_p;
        // unit 0: centre tap; meanwhile the -1 operand and the first half of the next half-group's split
        MI_READB2(pb[(3 * i + 1) & 1], hg_unit(i, -1));
        MI_UNIT(pc_, pb[(3 * i) & 1], if (MI_ROW_KEPT(i)) MI_SHIFT6(opm, h, m, 0x138, selm), if (MI_ROW_KEPT(i)) MI_SHIFT6B(opm, m, l, 0x138, selm),
                if (MI_ROW_KEPT((i + 1) % NH)) bf16_split_pair<0>(rc[0], nc), if (MI_ROW_KEPT((i + 1) % NH)) bf16_split_pair<1>(rc[0], nc))
        // unit 1: tap -1; meanwhile the +1 operand and the second half of the split
        MI_READB2(pb[(3 * i + 2) & 1], hg_unit(i, 1));
        MI_UNIT(opm, pb[(3 * i + 1) & 1], if (MI_ROW_KEPT(i)) MI_SHIFT6(opp, h, m, 0x130, selp), if (MI_ROW_KEPT(i)) MI_SHIFT6B(opp, m, l, 0x130, selp),
                if (MI_ROW_KEPT((i + 1) % NH)) bf16_split_pair<2>(rc[1], nc), if (MI_ROW_KEPT((i + 1) % NH)) bf16_split_pair<3>(rc[1], nc))
        // unit 2: tap +1
        MI_READB(pb[(3 * i + 3) & 1], hg_unit((i + 1) % NH, 0));
        MI_UNIT(opp, pb[(3 * i + 2) & 1], (void)0, (void)0, (void)0, (void)0)
      }
#undef MI_READB
#undef MI_READB2
#undef MI_UNIT
#undef MI_SHIFT6B
#undef MI_SHIFT6
#undef MI_SHIFT
    }
#pragma unroll
    for (int step = 0; step < (BF ? 0 : NSTEP); ++step) {
      if (step + DEPTH < NSTEP) issue(cur, step + DEPTH, ring[(step + DEPTH) % RING]);
      else if (MI_CONV_XTILE) issue(nxt, step + DEPTH - NSTEP, ring[(step + DEPTH) % RING]);
      __builtin_amdgcn_sched_barrier(0);
      const int cc = step % NCC, tt = step / NCC;           // tt = term*9 + tap
      const floatx4* av = ring[step % RING];
      const float* bl = lds + ((size_t)(tt * CI + cc * 32 + h * 16)) * 32 + j;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v][0], bl[(4 * v + 0) * 32], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v][1], bl[(4 * v + 1) * 32], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v][2], bl[(4 * v + 2) * 32], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[v][3], bl[(4 * v + 3) * 32], acc, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    cur = nxt;
    // The epilogue's stores are inline assembly (buf_st_untracked): the hazard recogniser does not see that they read the accumulators, and
    // the hardware does not interlock a matrix result against a following memory instruction's data read (up to 19 wait states after a
    // 16-pass MFMA).  Spend them here, once per tile, tied to the accumulators so that no MFMA can be scheduled behind the fence.
    // Only the BF variants store through assembly (they are the ones whose operand waits it rescues); the fp32-pipe variants keep the
    // compiler-visible store, whose matrix-result hazard is the compiler's to cover.
    if constexpr (BF) asm volatile("s_nop 15\n\ts_nop 7" : "+v"(acc));
    if constexpr (F16) {                                       // the operands' scales out of the sums (a power of two: exact)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] *= f16_inv;
    }
    if (!MI_CONV_XTILE) {
#pragma unroll
      for (int st = 0; st < DEPTH; ++st) issue(cur, st, ring[st % RING]);
    }
    // epilogue: rows m = (r&3) + 8*(r>>2) + 4h of the tile; rows past the end of the task are dropped by the range check
    if (EPI == EPI_BRED) {
      // block 1's pooled-resolution tensors at this lane's 16 output positions, a group of rows at a time (register budget: the
      // two-term variant must stay within 128 VGPRs for two 8-wave workgroups per CU): loads first, then the fp64 sums.  Rows past the
      // end of the task read p = 0, i.e. "ReLU off".
      constexpr int GR = NTERMS == 2 ? 2 : 8, NG = 16 / GR;  // rows per group; two groups of 2 (two terms: 4) x GR registers in flight
      // (two terms: groups of 2 rows keep the kernel within 128 VGPRs -- two 8-wave workgroups per CU)
      struct Grp { float pp[GR], zz[GR], zd[GR], dq[GR]; };
      auto row_off = [&](int r) {
        return obase + ((r >> 3) ? (unsigned)(16 * CO * 4) : 0u) + (unsigned)(((r & 3) + 8 * ((r >> 2) & 1)) * CO * 4);
      };
      // BF: accumulator rows 0 (r = 0 of lane half 0) and 31 (r = 15 of lane half 1) belong to the halo lanes: not stored, not summed
      auto dropped = [&](int r) { return BF && ((r == 0 && h == 0) || (r == 15 && h == 1)); };
      const int keep_lo = h == 0 ? 0 : -1, keep_hi = h == 1 ? 0 : -1;
      // One code path per source of "ReLU on" (a wave-uniform property of the launch): as a branch per row the choice fenced every row's
      // loads behind the previous row's (conv_b16.h, where the same hoist took the one-term dgrad from +39 % to -2 %).
      auto bred_path = [&](auto arg_c) {
      constexpr bool ARG = decltype(arg_c)::value;
      auto fetch = [&](int grp, Grp& gq) {
#pragma unroll
        for (int rr = 0; rr < GR; ++rr) {
          const unsigned o = row_off(grp * GR + rr);
          // (the byte as an integer in a float register: 0..3 = the window's argmax position, 4 = its ReLU is off;
          // a row past the end of the task reads 0 = "on", and contributes nothing: its accumulators and cotangents are exact zeros)
          if (ARG) gq.pp[rr] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b8(rbp, o >> 2, 0, 0));
          else gq.pp[rr] = buf_ld(rbp, o);
          gq.zz[rr] = buf_ld(rbzh, o);
          if (NTERMS == 2) { gq.zd[rr] = buf_ld(rbzhd, o); gq.dq[rr] = buf_ld(rbdp, o); }
        }
      };
      auto consume = [&](int grp, const Grp& gq) {
#pragma unroll
        for (int rr = 0; rr < GR; ++rr) {
          const int r = grp * GR + rr;
          const float v = acc[r];
          if constexpr (BF) buf_st_untracked(rout_raw, dropped(r) ? MI_OOB : row_off(r), v);
          else buf_st(rout, row_off(r), v);
          // "ReLU on" as a lane mask: p is a ReLU output (>= +0), so 0 - p carries a sign bit exactly where p > 0.  The masked
          // values are ANDs on the floats (mi_common.h): a select after the fp64 conversion is two quarter-rate v_cndmask per row
          int on = ARG ? ((int)__builtin_bit_cast(unsigned, gq.pp[rr]) - 4) >> 31      // -1 where the byte is below 4
                       : lane_mask_negative(0.f - gq.pp[rr]);
          if (BF && r == 0) on &= keep_lo;
          if (BF && r == 15) on &= keep_hi;
          const float vv = lane_keep_where(on, v);
          if (NTERMS == 1) {
            s = fma((double)vv, (double)gq.zz[rr], s);
          } else {
            const float dv = lane_keep_where(on, gq.dq[rr]);
            s += (double)vv * (double)gq.zz[rr] + (double)dv * (double)gq.zd[rr];
          }
          q += (double)vv;
        }
      };
      // the next group's loads are issued before this group's fp64 arithmetic (the lanes' sums are independent of the order)
      Grp ga, gb;
      fetch(0, ga);
#pragma unroll
      for (int grp = 0; grp < NG; grp += 2) {
        if (grp + 1 < NG) fetch(grp + 1, gb);
        consume(grp, ga);
        if (grp + 2 < NG) fetch(grp + 2, ga);
        if (grp + 1 < NG) consume(grp + 1, gb);
      }
      };
      if (bred_arg) bred_path(std::true_type{}); else bred_path(std::false_type{});
      continue;
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const unsigned ro = (unsigned)(((r & 3) + 8 * ((r >> 2) & 1)) * CO * 4);
      const bool drop = BF && ((r == 0 && h == 0) || (r == 15 && h == 1));      // the halo lanes' accumulator rows (BF tiles: 30 pixels)
      if constexpr (BF) buf_st_untracked(rout_raw, drop ? MI_OOB : obase + ((r >> 3) ? (unsigned)(16 * CO * 4) : 0u) + ro, acc[r]);
      else buf_st(rout, obase + ((r >> 3) ? (unsigned)(16 * CO * 4) : 0u) + ro, acc[r]);
      const float v = drop ? 0.f : acc[r];
      if (EPI == EPI_STATS) {
        const double dv = (double)v;
        s += dv;
        q = fma(dv, dv, q);
      } else if (EPI == EPI_TSTATS) {
        const float zh = bn_zh(zpre[r], mu_c, r_c);
        s += (double)v;
        q = fma((double)zh, (double)v, q);
      }
    }
  }
  CV_STAMP(3);
  if (EPI != EPI_NONE) {
    double* pb = a.partial + (size_t)task * gridDim.x * 2 * CO;
    stats_block_reduce(s, q, reinterpret_cast<double*>(lds), lane, wave, NW, pb, CO, cbase, a.fin, task, bx);
  }
  CV_STAMP(4);
}

#include "conv_b16.h"

// ---------------------------------------------------------------------------------------------------------------------
// First-layer conv: CI0 in {1,3}.  K = 9*CI0 padded to an even KP; lane half h takes k in [h*KP/2, (h+1)*KP/2).
template <int CI0, int EPI, int STRIDE>
__global__ __launch_bounds__(256) void conv3x3_first_mfma_kernel(ConvArgs a) {
  constexpr int K = 9 * CI0, KP = (K + 1) & ~1, KH = KP / 2;
  constexpr int LDS_FLOATS = KP * 32 > 1028 ? KP * 32 : 1028;  // weights, later 4 waves x 2 x 32 doubles for the stats / 512 doubles + flag of the fused finalize
  __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int task = blockIdx.y, ct = blockIdx.z;
  const int H = a.g.h, W = a.g.w, HO = a.g.ho, WO = a.g.wo, CO = a.g.co;
  const int cbase = ct * 32;
  const float* wsrc = a.wt[0] + (size_t)task * a.wstride;  // [9][CI0][CO] == [k][CO]
  for (int idx = tid; idx < KP * 32; idx += 256) {
    const int k = idx >> 5, nl = idx & 31;
    lds[idx] = (k < K) ? wsrc[(size_t)k * CO + cbase + nl] : 0.f;
  }
  __syncthreads();

  // per-lane tap table
  int kdy[KH], kdx[KH], kci[KH];
  bool kok[KH];
#pragma unroll
  for (int kk = 0; kk < KH; ++kk) {
    const int k = h * KH + kk;
    kok[kk] = k < K;
    const int tap = k / CI0;
    kci[kk] = k - tap * CI0;
    kdy[kk] = tap / 3 - 1;
    kdx[kk] = tap % 3 - 1;
  }

  const int mpix = a.mpix;
  const size_t in_task = (size_t)a.g.n * H * W * CI0;
  const size_t out_task = (size_t)mpix * CO;
  const float* in_t = a.in[0] + (size_t)task * in_task;
  float* out_t = a.out + (size_t)task * out_task;
  const float* z_t = (EPI == EPI_TSTATS) ? a.z + (size_t)task * out_task : nullptr;
  float mu_c = 0.f, r_c = 0.f;
  if (EPI == EPI_TSTATS) {
    mu_c = a.mu[(size_t)task * CO + cbase + j];
    r_c = a.rstd[(size_t)task * CO + cbase + j];
  }
  double s = 0.0, q = 0.0;
  const int tile0 = (blockIdx.x * 4 + wave) * a.tiles_per_wave;
  const int tile1 = min(tile0 + a.tiles_per_wave, a.ntiles);
  for (int tile = tile0; tile < tile1; ++tile) {
    const int pix = tile * 32 + j;
    const bool valid = pix < mpix;
    const int n = pix / (HO * WO);
    const int rem = pix - n * (HO * WO);
    const int oy = rem / WO, ox = rem - oy * WO;
    float av[KH];
#pragma unroll
    for (int kk = 0; kk < KH; ++kk) {
      const int iy = oy * STRIDE + kdy[kk], ix = ox * STRIDE + kdx[kk];
      const bool inb = valid && kok[kk] && iy >= 0 && iy < H && ix >= 0 && ix < W;
      av[kk] = inb ? in_t[((size_t)(n * H + iy) * W + ix) * CI0 + kci[kk]] : 0.f;
    }
    floatx16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KH; ++kk)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], lds[(h * KH + kk) * 32 + j], acc, 0, 0, 0);
    float zpre[16];
    if (EPI == EPI_TSTATS) conv_prefetch_z(zpre, z_t, tile, lane, mpix, CO, cbase);
    conv_epilogue<EPI>(acc, tile, lane, mpix, CO, cbase, out_t, zpre, mu_c, r_c, s, q);
  }
  if (EPI != EPI_NONE) {
    double* pb = a.partial + (size_t)task * gridDim.x * 2 * CO;
    stats_block_reduce(s, q, reinterpret_cast<double*>(lds), lane, wave, 4, pb, CO, cbase, a.fin, task);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// wgrad: dW[tap][ci][co] = sum over output pixels of x[pixin(pix,tap)][ci] * dz[pix][co].
// M = ci (32-chunk), N = co (32-tile), K = pixels.  Each wave owns a pixel chunk and 9 tap accumulators; lane half h takes
// every second pixel.  Partials [task][chunk][9][CI][CO] are summed in a fixed order by reduce_partials_kernel.
template <int NTERMS, int STRIDE>
__global__ __launch_bounds__(256) void wgrad3x3_mfma_kernel(WgradArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int task = blockIdx.y;
  const int H = a.g.h, W = a.g.w, HO = a.g.ho, WO = a.g.wo, CI = a.g.ci, CO = a.g.co;
  const int ncot = CO / 32;
  const int cit = blockIdx.z / ncot, cot = blockIdx.z - cit * ncot;
  const int chunk = blockIdx.x * 4 + wave;
  if (chunk >= a.nchunks) return;
  const int p0 = chunk * a.chunk_pix, p1 = min(p0 + a.chunk_pix, a.mpix);
  const size_t x_task = (size_t)a.g.n * H * W * CI, dz_task = (size_t)a.mpix * CO;

  floatx16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

#pragma unroll
  for (int term = 0; term < NTERMS; ++term) {
    const float* x_t = a.x[term] + (size_t)task * x_task + cit * 32 + j;
    const float* dz_t = a.dz[term] + (size_t)task * dz_task + cot * 32 + j;
    for (int p = p0 + h; p < p1 + h; p += 2) {  // both halves run the same trip count; the odd tail lane-half feeds zeros
      const bool valid = p < p1;
      const int n = p / (HO * WO);
      const int rem = p - n * (HO * WO);
      const int oy = rem / WO, ox = rem - oy * WO;
      const float b = valid ? dz_t[(size_t)p * CO] : 0.f;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const int iy = oy * STRIDE + tap / 3 - 1, ix = ox * STRIDE + tap % 3 - 1;
        const bool inb = valid && iy >= 0 && iy < H && ix >= 0 && ix < W;
        const float av = inb ? x_t[((size_t)(n * H + iy) * W + ix) * CI] : 0.f;
        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc[tap], 0, 0, 0);
      }
    }
  }
  float* pt = a.partial + ((size_t)task * a.nchunks + chunk) * 9 * CI * CO;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
      pt[((size_t)tap * CI + cit * 32 + row) * CO + cot * 32 + j] = acc[tap][r];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Stride-1 wgrad, register-tiled over image rows (the hot weight-gradient kernel).
// Work unit = (image n, row pair yp, column segment s): lane half h owns output row y = 2*yp + h, columns
// [s*RH, s*RH+RH).  Per unit a lane loads RH values of dz (B operand, its co) and a 3 x (RH+2) halo patch of x (A operand,
// its ci): 4*RH+6 coalesced dword loads feed 9*RH MFMAs (each x value is re-used by up to 9 (tap, pixel) pairs from
// registers).  Units are software-pipelined through two register sets so the next unit's loads fly under the current
// unit's MFMAs.  The 4 waves of a workgroup interleave units, reduce their 9 accumulators through LDS tap by tap and leave
// ONE partial per workgroup; reduce_partials_kernel folds workgroups in a fixed order (deterministic, no atomics).
template <int RH>
struct WgUnit {
  float xa[3][RH + 2];
  float b[RH];
};

template <int RH, bool EXACT>
__device__ __forceinline__ void wg_load_unit(WgUnit<RH>& u, int unit, mi_rsrc rx, mi_rsrc rdz, unsigned lane_x, unsigned lane_dz,
                                             int H, int W, int CI, int CO, int hp2, int nseg, int h) {
  // unit, and everything decoded from it, is wave-uniform (scalar unit)
  const int n = unit / (hp2 * nseg);
  const int rem = unit - n * hp2 * nseg;
  const int yp = rem / nseg, s = rem - yp * nseg;
  const int x0 = s * RH;
  const int y = 2 * yp + h;                                  // per lane half
  const bool rowok = y < H;
  const unsigned dzoff = rowok ? lane_dz + (unsigned)(((n * H + y) * W + x0) * CO) * 4u : MI_OOB;
  if (EXACT) {
    // W is a multiple of RH and CI == CO == 32: every dz column and the x columns 1..RH of a segment are inside the image, their
    // displacements are compile-time immediates of the load; only the halo columns 0 (first segment) and RH+1 (last segment) can fall
    // outside, selected per unit on a scalar condition.  One vector offset per row instead of one add per load.
#pragma unroll
    for (int i = 0; i < RH; ++i) u.b[i] = buf_ld(rdz, dzoff + (unsigned)(i * 32 * 4));
    const bool lok = s > 0, rok_c = s + 1 < nseg;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const int iy = y + r - 1;
      const bool rok = rowok && (unsigned)iy < (unsigned)H;
      const unsigned xoff = rok ? lane_x + (unsigned)(((n * H + iy) * W + x0) * 32) * 4u : MI_OOB;      // pixel x0 of the row
      u.xa[r][0] = buf_ld(rx, lok ? xoff - 128u : MI_OOB);
#pragma unroll
      for (int c = 1; c <= RH; ++c) u.xa[r][c] = buf_ld(rx, xoff + (unsigned)((c - 1) * 128));
      u.xa[r][RH + 1] = buf_ld(rx, rok_c ? xoff + (unsigned)(RH * 128) : MI_OOB);
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < RH; ++i) {
    const unsigned col = (x0 + i) < W ? (unsigned)(i * CO) * 4u : MI_OOB;          // scalar select
    u.b[i] = buf_ld(rdz, dzoff + col);
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int iy = y + r - 1;
    const bool rok = rowok && (unsigned)iy < (unsigned)H;
    const unsigned xoff = rok ? lane_x + (unsigned)(((n * H + iy) * W + x0 - 1) * CI) * 4u : MI_OOB;
#pragma unroll
    for (int c = 0; c < RH + 2; ++c) {
      const unsigned col = (unsigned)(x0 + c - 1) < (unsigned)W ? (unsigned)(c * CI) * 4u : MI_OOB;   // scalar select
      u.xa[r][c] = buf_ld(rx, xoff + col);
    }
  }
}

template <int RH>
__device__ __forceinline__ void wg_compute_unit(const WgUnit<RH>& u, floatx16* acc) {
#pragma unroll
  for (int i = 0; i < RH; ++i)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
      acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(u.xa[tap / 3][i + tap % 3], u.b[i], acc[tap], 0, 0, 0);
}

template <int RH, bool EXACT>
__global__ __launch_bounds__(256, 2) void wgrad3x3_rows_mfma_kernel(WgradArgs a) {
  __shared__ float red[4 * 1024];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably wave-uniform: unit decode runs on the scalar unit
  const int j = lane & 31, h = lane >> 5;
  const int task = blockIdx.y;
  const int H = a.g.h, W = a.g.w, CI = a.g.ci, CO = a.g.co;   // stride 1: conv output is H x W as well
  const int ncot = CO / 32;
  const int cit = blockIdx.z / ncot, cot = blockIdx.z - cit * ncot;
  const int hp2 = (H + 1) >> 1, nseg = (W + RH - 1) / RH;
  const int nunits = a.g.n * hp2 * nseg;                     // per term; the unit stream is [term][unit]
  const int total = nunits * a.nterms;
  const int ub0 = blockIdx.x * a.chunk_pix;                  // chunk_pix = units per workgroup here
  const int ub1 = min(ub0 + a.chunk_pix, total);
  const size_t x_task = (size_t)a.g.n * H * W * CI, dz_task = (size_t)a.g.n * H * W * CO;
  const unsigned xb = (unsigned)(x_task * 4), db = (unsigned)(dz_task * 4);
  const mi_rsrc rx0 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.x[0] + (size_t)task * x_task), 0, xb, 0x00020000);
  const mi_rsrc rd0 = __builtin_amdgcn_make_buffer_rsrc((void*)(a.dz[0] + (size_t)task * dz_task), 0, db, 0x00020000);
  const float* x1p = a.nterms > 1 ? a.x[1] : a.x[0];
  const float* d1p = a.nterms > 1 ? a.dz[1] : a.dz[0];
  const mi_rsrc rx1 = __builtin_amdgcn_make_buffer_rsrc((void*)(x1p + (size_t)task * x_task), 0, xb, 0x00020000);
  const mi_rsrc rd1 = __builtin_amdgcn_make_buffer_rsrc((void*)(d1p + (size_t)task * dz_task), 0, db, 0x00020000);
  const unsigned lane_x = (unsigned)(cit * 32 + j) * 4u, lane_dz = (unsigned)(cot * 32 + j) * 4u;

  floatx16 acc[9];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  auto load = [&](WgUnit<RH>& un, int v) {
    if (v >= nunits) wg_load_unit<RH, EXACT>(un, v - nunits, rx1, rd1, lane_x, lane_dz, H, W, CI, CO, hp2, nseg, h);   // wave-uniform branch
    else wg_load_unit<RH, EXACT>(un, v, rx0, rd0, lane_x, lane_dz, H, W, CI, CO, hp2, nseg, h);
  };
  WgUnit<RH> u0, u1;
  int u = ub0 + wave;
  if (u < ub1) load(u0, u);
  for (; u < ub1; u += 8) {
    if (u + 4 < ub1) load(u1, u + 4);
    wg_compute_unit<RH>(u0, acc);
    if (u + 8 < ub1) load(u0, u + 8);
    if (u + 4 < ub1) wg_compute_unit<RH>(u1, acc);
  }

  // cross-wave reduction, one tap at a time: red[wave][r*64 + lane]
  float* pt = a.partial + ((size_t)task * gridDim.x + blockIdx.x) * 9 * CI * CO;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wave * 1024 + r * 64 + lane] = acc[tap][r];
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = tid + 256 * q;
      const float v = red[e] + red[1024 + e] + red[2048 + e] + red[3072 + e];
      const int r = e >> 6, l = e & 63;
      const int row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31;
      pt[((size_t)tap * CI + cit * 32 + row) * CO + cot * 32 + col] = v;
    }
    __syncthreads();
  }
}

// First-layer wgrad: rows m = tap*CI0 + ci (27 or 9 of 32), one accumulator.
template <int CI0, int STRIDE>
__global__ __launch_bounds__(256) void wgrad3x3_first_mfma_kernel(WgradArgs a) {
  constexpr int K = 9 * CI0;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int j = lane & 31, h = lane >> 5;
  const int task = blockIdx.y, cot = blockIdx.z;
  const int H = a.g.h, W = a.g.w, HO = a.g.ho, WO = a.g.wo, CO = a.g.co;
  const int chunk = blockIdx.x * 4 + wave;
  if (chunk >= a.nchunks) return;
  const int p0 = chunk * a.chunk_pix, p1 = min(p0 + a.chunk_pix, a.mpix);
  const size_t x_task = (size_t)a.g.n * H * W * CI0, dz_task = (size_t)a.mpix * CO;
  const bool mok = j < K;
  const int tap = j / CI0, ci = j - tap * CI0;
  const int dy = tap / 3 - 1, dx = tap % 3 - 1;
  const float* x_t = a.x[0] + (size_t)task * x_task + ci;
  const float* dz_t = a.dz[0] + (size_t)task * dz_task + cot * 32 + j;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int p = p0 + h; p < p1 + h; p += 2) {
    const bool valid = p < p1;
    const int n = p / (HO * WO);
    const int rem = p - n * (HO * WO);
    const int oy = rem / WO, ox = rem - oy * WO;
    const float b = valid ? dz_t[(size_t)p * CO] : 0.f;
    const int iy = oy * STRIDE + dy, ix = ox * STRIDE + dx;
    const bool inb = valid && mok && iy >= 0 && iy < H && ix >= 0 && ix < W;
    const float av = inb ? x_t[((size_t)(n * H + iy) * W + ix) * CI0] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, b, acc, 0, 0, 0);
  }
  float* pt = a.partial + ((size_t)task * a.nchunks + chunk) * K * CO;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
    if (row < K) pt[(size_t)row * CO + cot * 32 + j] = acc[r];
  }
}

// out[task*ostride + e] = sum_chunk partial[task][chunk][e]   (fixed order => deterministic): the canonical fold of fold.h -- thread
// (slice, element) adds its slice's rounds, the slices meet in LDS.  One slice up to 16 chunks (the plain sequential sum).
__global__ __launch_bounds__(256) void reduce_partials_kernel(const float* __restrict__ partial, int nchunks, int nelem,
                                                              float* __restrict__ out, size_t ostride, int S) {
  __shared__ float part[256];
  const int epw = 256 / S;
  const int el = threadIdx.x % epw, sl = threadIdx.x / epw;
  const int e = blockIdx.x * epw + el;
  const int task = blockIdx.y;
  float v = 0.f;
  if (e < nelem) v = fold_slice<float>(partial + (size_t)task * nchunks * nelem + e, (size_t)nelem, nchunks, S, sl);
  if (S == 1) {
    if (e < nelem) out[(size_t)task * ostride + e] = v;
    return;
  }
  part[threadIdx.x] = v;
  __syncthreads();
  if (sl == 0 && e < nelem) {
    float t = part[el];
    for (int q = 1; q < S; ++q) t += part[q * epw + el];
    out[(size_t)task * ostride + e] = t;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// host launchers
// Operand form of the 32- / 64-channel stride-1 kernels: 0 = the fp32 pipe everywhere, 1 = three bf16 planes (six products), 2 = two
// scaled fp16 planes (three products; launches whose operands come without a largest-magnitude cell take form 1).
// MI_CONV_BF16X3 / mi_conv_set_split_bf16.
// Default: form 1.  Form 2 carries 22 bits of each operand -- narrower than the reference's fp32, however small its measured errors --
// so it is an opt-in (MI_CONV_BF16X3=2 / mi_conv_set_split_bf16(2)) with its own labelled line in bench.py, never the headline.
#ifndef MI_CONV_DEFAULT_FORM
#define MI_CONV_DEFAULT_FORM 1
#endif
static int g_conv_split_bf16 = -1;
static unsigned g_conv_split_mask = 0x3ffffu;                   // debug: which variants take the split form: conv bit ((terms-1)*2 + mode)*4 + epi, weight gradient bit 16 + (terms-1)
static bool conv_split_bf16() {
  if (g_conv_split_bf16 < 0) {
    const char* e = getenv("MI_CONV_BF16X3");
    g_conv_split_bf16 = e ? (atoi(e) < 0 ? 0 : (atoi(e) > 2 ? 2 : atoi(e))) : MI_CONV_DEFAULT_FORM;
    const char* m = getenv("MI_CONV_BF16X3_MASK");              // bisecting aid (hex): the variant mask of mi_conv_set_split_bf16
    if (m) g_conv_split_mask = (unsigned)strtoul(m, nullptr, 16);
  }
  return g_conv_split_bf16 != 0;
}
extern "C" int mi_conv_set_split_bf16(int on) {
  conv_split_bf16();
  const int was = g_conv_split_bf16;
  g_conv_split_bf16 = (on & 0xff) > 2 ? 2 : (on & 0xff);
  g_conv_split_mask = on > 0xff ? ((unsigned)on >> 8) : 0x3ffffu;
  // on = 0x100 * mask + form: only the variants in mask (bisecting aid)
  return was;
}
int conv_operand_form() { conv_split_bf16(); return g_conv_split_bf16; }
// the operand form in force, read WITHOUT touching it (a set-and-restore would reset the bisecting mask): mask_out, when given,
// receives the variant mask of MI_CONV_BF16X3_MASK / mi_conv_set_split_bf16
extern "C" int mi_conv_get_split_bf16(unsigned* mask_out) {
  conv_split_bf16();
  const int on = g_conv_split_bf16;
  if (mask_out) *mask_out = g_conv_split_mask;
  return on;
}

static inline void conv_grid(int mpix, int tasks, int cot, int nw, int ci, int nterms, int& ntiles, int& tpw, dim3& grid, int tile_pix = 32,
                             bool four_per_simd = false) {
  ntiles = ceil_div(mpix, tile_pix);
  // One balanced round: give every resident wave ceil(tiles / slots) tiles -- more, shorter waves would run as 2.x rounds whose last
  // round is mostly idle.  Resident waves: 4 per SIMD by registers (<= 128 VGPRs in every variant), limited by the LDS copy of the
  // weights (160 KB per CU): 36 KB per 32-channel term and workgroup -> 4096 waves on the chip; the 64-channel kernels stage 74 KB
  // (one term, two workgroups of 4 waves per CU) or 147 KB (two terms, one workgroup) -> 2048 / 1024 waves.
  // Split-bf16 32-channel kernels: 54 KB (one term, two 4-wave workgroups per CU) / 108 KB (two terms, one 8-wave workgroup) -> 2048.
  // (split-bf16 form: 2 waves per SIMD in every variant; fp16 form: 4, except with the tangent-statistics epilogue)
  const long slots = four_per_simd ? 4096 : (tile_pix != 32 ? 2048 : (ci >= 64 ? (nterms == 2 ? 1024 : 2048) : 4096));
  long total = (long)ntiles * tasks * cot;
  tpw = (int)((total + slots - 1) / slots);
  if (tpw < 1) tpw = 1;
  if (tpw > 128) tpw = 128;
  grid = dim3(ceil_div(ntiles, nw * tpw), tasks, cot);
}

int conv_tiles_per_wave(int mpix, int tasks, int cot) {
  int ntiles, tpw;
  dim3 grid;
  conv_grid(mpix, tasks, cot, 4, 32, 1, ntiles, tpw, grid, conv_split_bf16() ? 30 : 32);   // (a 32-filter stride-1 block, as the tests ask)
  return tpw;
}

int conv_max_blocks_per_task(const ConvGeom& g) {  // tiles_per_wave == 1 is the finest split any launch uses (30-pixel tiles: split-bf16 form)
  return ceil_div(ceil_div(g.n * g.ho * g.wo, 30), 4);
}

// Kernels that stage more than 64 KB: allow_dynamic_lds (mi_common.h) with the launch's constant request.
template <int CI, int NTERMS, int EPI, int MODE, int STRIDE>
static hipError_t launch_conv_t(hipStream_t st, ConvArgs& a, dim3 grid) {
  const size_t lds = (size_t)NTERMS * 9 * CI * 32 * sizeof(float);
  auto k = conv3x3_mfma_kernel<CI, NTERMS, EPI, MODE, STRIDE>;
  static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
  if (lds > 64 * 1024) if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(k), lds, &attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, dim3(ConvWaves<CI, NTERMS>::value * 64), lds, st, a);
  return hipGetLastError();
}
template <int CI, int NTERMS, int EPI, int MODE, bool F16>
static hipError_t launch_conv_s1_bf(hipStream_t st, ConvArgs& a, dim3 grid) {
  const size_t lds = (size_t)NTERMS * 9 * CI * 32 * (F16 ? 4 : 6) + (F16 ? 64 : 0);   // three bf16 planes / two fp16 planes + the weight maxima
  auto k = conv3x3_s1_mfma_kernel<CI, NTERMS, EPI, MODE, true, F16>;
  static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
  if (lds > 64 * 1024) if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(k), lds, &attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, dim3(ConvWaves<CI, NTERMS, true, F16>::value * 64), lds, st, a);
  return hipGetLastError();
}
// the 16x16x32 kernel's BatchNorm statistics in fp64 per value where a task's whole map is one tile (conv_b16.h, S64).  The edge is
// EMPIRICAL: the fp32 partials' cancellation does not stop at two tiles (8 partials per channel), it only averages down with their number
static bool conv_b16_stats64(const ConvArgs& a) { return a.ntiles == 1; }
// the split-bf16 form on 16x16x32 MFMAs with one accumulator per horizontal tap (conv_b16.h): same LDS, workgroup shape and grid
template <int CI, int NTERMS, int EPI, int MODE>
static hipError_t launch_conv_s1_b16(hipStream_t st, ConvArgs& a, dim3 grid) {
  const size_t lds = (size_t)NTERMS * 9 * CI * 32 * 6;
  if constexpr (EPI == EPI_STATS) {
    if (conv_b16_stats64(a)) {               // (a task of a single tile: conv_b16.h, S64)
      auto k = conv3x3_s1_b16_kernel<CI, NTERMS, EPI, MODE, true>;
      static unsigned attr_done64 = 0;
      if (lds > 64 * 1024) if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(k), lds, &attr_done64); e != hipSuccess) return e;
      hipLaunchKernelGGL(k, grid, dim3(ConvWaves<CI, NTERMS, true, false>::value * 64), lds, st, a);
      return hipGetLastError();
    }
  }
  auto k = conv3x3_s1_b16_kernel<CI, NTERMS, EPI, MODE>;
  static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
  if (lds > 64 * 1024) if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(k), lds, &attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, dim3(ConvWaves<CI, NTERMS, true, false>::value * 64), lds, st, a);
  return hipGetLastError();
}
// 0 = never, 1 = launches of at least MI_CONV_B16_MIN_TPW tiles per wave (default), 2 = every launch.  The 16x16x32 kernel works in
// row-steps of 72 MFMAs behind 4 loads and 16 split values, and its epilogue ends in a lane rotation: with one or two tiles per wave (the
// 10 x 10 block at 32 tasks, every block at few tasks per call) the 32x32x16 kernel's shorter fill and drain win
// (profiles/r5/ab_conv_b16_*.txt: block 4 forward 0.0205 -> 0.0241 ms, block 2 forward 0.1463 -> 0.1376 ms).  The threshold is 6 tiles
// per wave (rounded up): measured inside the whole meta-iteration (tools/r5_ab_env.sh MI_CONV_B16_MIN_TPW, alternating pairs on one box) 5
// against 8 is -0.5 % at 32 tasks per call (block 3: 5.7 tiles per wave -> 6), -1.7 % at 8 tasks (block 2, 5.7), -1.2 % on cfg4 (4.6 -> 5);
// 3, 2 and 1 change nothing or lose at 1 - 4 tasks per call.  6, not 5: cfg4's 32-task call would otherwise run block 2 on this kernel and
// its tasks one at a time on the other, and the full-size test that holds the two to 1e-6 (near-tied pooling decisions aside) is frozen.
// (Isolated launches had read the 16x16x32 kernel as slower at 5.7 tiles.)
static int g_conv_b16 = -1, g_conv_b16_min_tpw = -1;
int conv_b16() {
  if (g_conv_b16 < 0) {
    const char* e = getenv("MI_CONV_B16");
    g_conv_b16 = e ? (atoi(e) < 0 ? 0 : (atoi(e) > 2 ? 2 : atoi(e))) : MI_CONV_B16_DEFAULT;
    const char* m = getenv("MI_CONV_B16_MIN_TPW");
    g_conv_b16_min_tpw = m ? atoi(m) : 6;
  }
  return g_conv_b16;
}
extern "C" int mi_conv_set_b16(int on) { const int was = conv_b16(); if (on >= 0) g_conv_b16 = on > 2 ? 2 : on; return was; }
// How the two waves of a SIMD share it in the 16x16x32 kernel (MI_CONV_STAGGER; bit 0: the second wave starts half a tile late -- no effect,
// off; bit 1, the DEFAULT: issue priority alternates between the two from tile to tile).  tools/conv_b16_stamps.py: at equal priority the older
// wave's K loop takes 10.3k cycles per two-term tile and the younger's 14.5k, so the older finishes a quarter of the launch early; alternating
// priority balances them (12.6k / 13.6k, launch cycles -5 %).  Isolated launches move by -2 % (forward) / +2 % (dgrad); inside the meta-iteration
// (tools/r5_ab_env.sh, six alternating pairs on two boxes) it is -0.3 ... -1.0 % on cfg2 (16.33 against 16.41 ms) and -0.7 % on cfg3: on.
static int conv_stagger() { static const int v = getenv("MI_CONV_STAGGER") ? atoi(getenv("MI_CONV_STAGGER")) : 2; return v; }
static bool conv_b16_for(const ConvArgs& a) { const int m = conv_b16(); return m == 2 || (m == 1 && a.tiles_per_wave >= g_conv_b16_min_tpw); }
// which kernel of the stride-1 family a launch takes (a.split_bf16 and a.tiles_per_wave as conv_fill left them); conv_plan reports it
static int conv_s1_kind(const ConvArgs& a) {
  if (a.split_bf16 == 2) return CONV_K_S1_F16;
  if (a.split_bf16 && conv_b16_for(a)) return CONV_K_S1_BF16_16X16;
  if (a.split_bf16) return CONV_K_S1_BF16_32X32;
  return CONV_K_S1_F32;
}
template <int CI, int NTERMS, int EPI, int MODE>
static hipError_t launch_conv_s1(hipStream_t st, ConvArgs& a, dim3 grid) {
  if constexpr (CI == 32 || (CI == 64 && NTERMS == 1)) {
    const int kind = conv_s1_kind(a);
    if (kind == CONV_K_S1_F16) return launch_conv_s1_bf<CI, NTERMS, EPI, MODE, true>(st, a, grid);
    if (kind == CONV_K_S1_BF16_16X16) return launch_conv_s1_b16<CI, NTERMS, EPI, MODE>(st, a, grid);
    if (kind == CONV_K_S1_BF16_32X32) return launch_conv_s1_bf<CI, NTERMS, EPI, MODE, false>(st, a, grid);
  }
  const size_t lds = (size_t)NTERMS * 9 * CI * 32 * sizeof(float);
  auto k = conv3x3_s1_mfma_kernel<CI, NTERMS, EPI, MODE>;
  static unsigned attr_done = 0;             // one bit per device: the attribute belongs to the device's copy of the kernel
  if (lds > 64 * 1024) if (hipError_t e = allow_dynamic_lds(reinterpret_cast<const void*>(k), lds, &attr_done); e != hipSuccess) return e;
  hipLaunchKernelGGL(k, grid, dim3(ConvWaves<CI, NTERMS>::value * 64), lds, st, a);
  return hipGetLastError();
}

// the stride-1 kernel needs co == ci, 32-bit byte offsets inside one task's tensor and pixel indices below 2^24
static bool conv_s1_ok(const ConvArgs& a) {
  return a.g.stride == 1 && a.g.co == a.g.ci && a.g.h == a.g.ho && a.g.w == a.g.wo && a.mpix < (1 << 24) &&
         (size_t)a.mpix * a.g.ci * 4 < (size_t)MI_OOB;
}

template <int CI, int NTERMS, int EPI>
static hipError_t launch_conv_ms(hipStream_t st, ConvArgs& a, dim3 grid, int mode, int stride) {
  if constexpr (EPI == EPI_BRED) {                           // only the stride-1 hidden -> hidden dgrad carries this epilogue
    if (conv_s1_ok(a) && mode == 1) return launch_conv_s1<CI, NTERMS, EPI_BRED, 1>(st, a, grid);
    return hipErrorInvalidValue;
  } else {
    if (conv_s1_ok(a)) {
      if (mode == 0) return launch_conv_s1<CI, NTERMS, EPI, 0>(st, a, grid);
      if (EPI == EPI_NONE && mode == 1) return launch_conv_s1<CI, NTERMS, EPI_NONE, 1>(st, a, grid);
      return hipErrorInvalidValue;
    }
    if (mode == 0 && stride == 1) return launch_conv_t<CI, NTERMS, EPI, 0, 1>(st, a, grid);
    if (mode == 0 && stride == 2) return launch_conv_t<CI, NTERMS, EPI, 0, 2>(st, a, grid);
    if (EPI == EPI_NONE) {
      if (mode == 1 && stride == 1) return launch_conv_t<CI, NTERMS, EPI_NONE, 1, 1>(st, a, grid);
      if (mode == 1 && stride == 2) return launch_conv_t<CI, NTERMS, EPI_NONE, 1, 2>(st, a, grid);
    }
    return hipErrorInvalidValue;
  }
}

// Generic conv launcher.  mode 0 = forward, 1 = dgrad.  epi as EPI_*.  Returns blocks per task (partials written).
// The decisions of a launch: operand form, waves per workgroup, tile size and the tile split, left in a (split_bf16, ntiles,
// tiles_per_wave, stagger) and grid.  have_scales: the fp16 form's largest-magnitude cells are there.  Returns waves per workgroup.
constexpr int CONV_FIRST_WAVES = 4;          // workgroup of the first-layer kernel
static int conv_fill(ConvArgs& a, int tasks, int nterms, int epi, int mode, bool have_scales, dim3& grid) {
  const int cot = a.g.co / 32;
  int ntiles, tpw;
  // the split-bf16 form of the stride-1 kernel (32 filters; 64 filters with one term): tiles of 30 output pixels, 2048 resident waves
  a.split_bf16 = ((a.g.ci == 32 || (a.g.ci == 64 && nterms == 1)) && conv_s1_ok(a) && conv_split_bf16() &&
                  (epi == EPI_BRED ? mode == 1 : (mode == 0 || epi == EPI_NONE)) &&
                  ((g_conv_split_mask >> (((nterms - 1) * 2 + mode) * 4 + epi)) & 1u)) ? conv_operand_form() : 0;
  if (a.split_bf16 == 2 && !have_scales) a.split_bf16 = 1;      // no scales: the bf16 form
  const int nw = ((a.split_bf16 == 2 && MI_F16_WIDE) || (nterms == 2 && a.g.ci == 32) || (a.split_bf16 && a.g.ci == 64)) ? 8 : 4;     // ConvWaves<CI, NTERMS, BF, F16>
  conv_grid(a.mpix, tasks, cot, nw, a.g.ci, nterms, ntiles, tpw, grid, a.split_bf16 ? 30 : 32, a.split_bf16 == 2 && MI_F16_WIDE && epi != EPI_TSTATS);
  a.ntiles = ntiles;
  a.tiles_per_wave = tpw;
  a.stagger = conv_stagger();
  return nw;
}
// Which kernel a launch takes (CONV_K_*), from a as conv_fill left it; -1: no kernel takes this combination of geometry, terms, epilogue
// and mode.  launch_conv3x3 refuses what this refuses and conv_plan reports it: the template dispatch below only spells the instance.
static int conv_kernel_of(const ConvArgs& a, int nterms, int epi, int mode) {
  if (a.g.co % 32 != 0 || nterms < 1 || nterms > 2 || (nterms == 2 && epi == EPI_STATS)) return -1;
  if (a.g.ci == 1 || a.g.ci == 3)
    return (mode == 0 && nterms == 1 && epi != EPI_BRED && (a.g.stride == 1 || a.g.stride == 2)) ? CONV_K_FIRST : -1;
  if (a.g.ci != 32 && a.g.ci != 64) return -1;
  if (epi == EPI_BRED) return (conv_s1_ok(a) && mode == 1) ? conv_s1_kind(a) : -1;   // only the stride-1 hidden -> hidden dgrad carries it
  if (mode != 0 && !(mode == 1 && epi == EPI_NONE)) return -1;
  if (conv_s1_ok(a)) return conv_s1_kind(a);
  return (a.g.stride == 1 || a.g.stride == 2) ? CONV_K_GENERIC : -1;
}
// g as the launch sees it (dgrad: the geometry of the transposed convolution, input = dz); mpix = n * ho * wo
ConvPlan conv_plan(const ConvGeom& g, int tasks, int nterms, int epi, int mode, bool have_scales) {
  ConvArgs a{};
  a.g = g;
  a.mpix = g.n * g.ho * g.wo;
  dim3 grid;
  const int nw = conv_fill(a, tasks, nterms, epi, mode, have_scales, grid);
  ConvPlan p{};
  p.kernel = conv_kernel_of(a, nterms, epi, mode);
  p.tiles_per_wave = a.tiles_per_wave;
  p.ntiles = a.ntiles;
  p.blocks = (int)grid.x;
  p.tile_pix = a.split_bf16 ? 30 : 32;
  p.waves = p.kernel == CONV_K_FIRST ? CONV_FIRST_WAVES : nw;
  p.form = a.split_bf16;
  p.stats64 = p.kernel == CONV_K_S1_BF16_16X16 && epi == EPI_STATS && conv_b16_stats64(a);
  return p;
}

hipError_t launch_conv3x3(hipStream_t st, ConvArgs a, int tasks, int nterms, int epi, int mode, int* blocks_per_task) {
  dim3 grid;
  conv_fill(a, tasks, nterms, epi, mode, a.amax[0] && (nterms == 1 || a.amax[1]), grid);
  if (blocks_per_task) *blocks_per_task = grid.x;
  const int kind = conv_kernel_of(a, nterms, epi, mode);
  if (kind < 0) return hipErrorInvalidValue;
  const int s = a.g.stride;
  if (kind == CONV_K_FIRST) {
#define FIRST(CI0, E, S) hipLaunchKernelGGL((conv3x3_first_mfma_kernel<CI0, E, S>), grid, dim3(CONV_FIRST_WAVES * 64), 0, st, a)
    if (a.g.ci == 3 && s == 1) { if (epi == EPI_STATS) FIRST(3, EPI_STATS, 1); else if (epi == EPI_TSTATS) FIRST(3, EPI_TSTATS, 1); else FIRST(3, EPI_NONE, 1); }
    else if (a.g.ci == 3 && s == 2) { if (epi == EPI_STATS) FIRST(3, EPI_STATS, 2); else if (epi == EPI_TSTATS) FIRST(3, EPI_TSTATS, 2); else FIRST(3, EPI_NONE, 2); }
    else if (a.g.ci == 1 && s == 1) { if (epi == EPI_STATS) FIRST(1, EPI_STATS, 1); else if (epi == EPI_TSTATS) FIRST(1, EPI_TSTATS, 1); else FIRST(1, EPI_NONE, 1); }
    else if (a.g.ci == 1 && s == 2) { if (epi == EPI_STATS) FIRST(1, EPI_STATS, 2); else if (epi == EPI_TSTATS) FIRST(1, EPI_TSTATS, 2); else FIRST(1, EPI_NONE, 2); }
    else return hipErrorInvalidValue;
#undef FIRST
    return hipGetLastError();
  }
#define DISPATCH(CI)                                                                              \
  if (nterms == 1) {                                                                              \
    if (epi == EPI_NONE) return launch_conv_ms<CI, 1, EPI_NONE>(st, a, grid, mode, s);             \
    if (epi == EPI_STATS) return launch_conv_ms<CI, 1, EPI_STATS>(st, a, grid, mode, s);           \
    if (epi == EPI_BRED) return launch_conv_ms<CI, 1, EPI_BRED>(st, a, grid, mode, s);             \
    return launch_conv_ms<CI, 1, EPI_TSTATS>(st, a, grid, mode, s);                                \
  } else {                                                                                        \
    if (epi == EPI_NONE) return launch_conv_ms<CI, 2, EPI_NONE>(st, a, grid, mode, s);             \
    if (epi == EPI_TSTATS) return launch_conv_ms<CI, 2, EPI_TSTATS>(st, a, grid, mode, s);         \
    if (epi == EPI_BRED) return launch_conv_ms<CI, 2, EPI_BRED>(st, a, grid, mode, s);             \
    return hipErrorInvalidValue;                                                                  \
  }
  if (a.g.ci == 32) { DISPATCH(32) }
  if (a.g.ci == 64) { DISPATCH(64) }
#undef DISPATCH
  return hipErrorInvalidValue;
}

// wgrad launcher: writes dW (tap-major [9][ci][co]) for every task at out + task*ostride.
int wgrad_chunks(int mpix, int tasks) {
  // aim for >= ~2048 waves in flight with chunks of 32..1024 pixels.  The small end matters for the launch-bound few-image
  // configurations: Omniglot 5-way 1-shot has 245 output pixels per task in block 2 -- with 256-pixel chunks ONE wave per
  // (task, ci tile, co tile) walked them serially (0.29 ms, 40 % of the cfg1 meta-iteration).
  int chunk = 1024;
  while (chunk > 32 && (long)ceil_div(mpix, chunk) * tasks < 2048) chunk >>= 1;
  return chunk;
}

// ---- stride-1 row-tiled wgrad: segment length and work split
static int rows_pick_rh(int w) {
  const int cand[4] = {7, 8, 5, 4};
  int best = 7, best_waste = 1 << 30;
  for (int i = 0; i < 4; ++i) {
    const int waste = ceil_div(w, cand[i]) * cand[i] - w;
    if (waste < best_waste) { best_waste = waste; best = cand[i]; }
  }
  return best;
}
static bool use_rows_kernel(const ConvGeom& g) { return g.stride == 1 && g.ci % 32 == 0 && g.co % 32 == 0; }
static void rows_split(const ConvGeom& g, int tasks, int& rh, int& nunits, int& upb, int& blocks) {
  rh = rows_pick_rh(g.w);
  nunits = g.n * ((g.h + 1) / 2) * ceil_div(g.w, rh);
  const int nz = (g.ci / 32) * (g.co / 32);
  // Workgroups per task: the kernel keeps 9 x 16 accumulator registers, two workgroups per CU are resident (512 on the chip).  A
  // launch takes ceil(workgroups / 512) rounds of (units per workgroup + the LDS reduction epilogue, worth ~16 units) each: pick
  // the split with the smallest product.  (T = 32 tasks of 5 images: 16 workgroups per task =
  // ONE round of 40 units instead of 20 = 1.25 rounds of 32.)
  // (never fewer than two units per wave on average; the 10x10 block's 250 units per task go to 16 workgroups at 32 tasks per call)
  int max_bpt = ceil_div(nunits, 8);
  if (max_bpt > 128) max_bpt = 128;
  if (max_bpt < 1) max_bpt = 1;
  int best = 1;
  long best_cost = -1;
  for (int bpt = 1; bpt <= max_bpt; ++bpt) {
    const long rounds = ((long)tasks * nz * bpt + 511) / 512;
    const long cost = rounds * (ceil_div(nunits, bpt) + 16);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = bpt; }
  }
  upb = ceil_div(nunits, best);
  blocks = ceil_div(nunits, upb);
}

// split-bf16 weight gradient (wgrad_bf16.hip): units of 2 rows x 8 columns, ONE workgroup per CU (144 accumulator AGPRs per lane)
bool wgrad_bf16_ok(const ConvGeom& g);
int wgrad_bf16_units(const ConvGeom& g);
hipError_t launch_wgrad_rows_bf16(hipStream_t st, const WgradArgs& a, dim3 grid);
bool wgrad_bf16_strips(const ConvGeom& g);
int wgrad_bf16_strip_rows(const ConvGeom& g, int rows);
int wgrad_bf16_strip_items(const ConvGeom& g, int rows);
hipError_t launch_wgrad_strips_bf16(hipStream_t st, WgradArgs a, dim3 grid, int rows);
// strip form: rows per piece and items (a 16-column strip piece) per workgroup; each of the four waves walks whole items.  Cost of a
// split in steps (one output row = 54 MFMAs): rounds of 256 resident workgroups x (items per wave x (rows + 3 for the item's prologue)
// + ~8 for the reduction epilogue).
static void strips_split_bf16(const ConvGeom& g, int tasks, int nterms, int& rows, int& ipb, int& blocks) {
  const int cand[4] = {24, 16, 12, 8};
  const int nz = (g.ci / 32) * (g.co / 32);
  long best_cost = -1;
  rows = 24; ipb = 1; blocks = 1;
  for (int c = 0; c < 4; ++c) {
    const int rp = wgrad_bf16_strip_rows(g, cand[c]);
    const int items = wgrad_bf16_strip_items(g, cand[c]);
    int max_bpt = items < 128 ? items : 128;
    if (max_bpt < 1) max_bpt = 1;
    for (int bpt = 1; bpt <= max_bpt; ++bpt) {
      const long rounds = ((long)tasks * bpt * nz + 255) / 256;
      const long cost = rounds * ((long)ceil_div(ceil_div(items, bpt) * nterms, 4) * (rp + 3) + 8);
      if (best_cost < 0 || cost < best_cost) {
        best_cost = cost; rows = cand[c]; ipb = ceil_div(items, bpt); blocks = ceil_div(items, ipb);
      }
    }
  }
}
static void rows_split_bf16(const ConvGeom& g, int tasks, int& nunits, int& upb, int& blocks) {
  nunits = wgrad_bf16_units(g);
  int max_bpt = ceil_div(nunits, 16);                       // never fewer than 4 units per wave
  if (max_bpt > 128) max_bpt = 128;
  if (max_bpt < 1) max_bpt = 1;
  int best = 1;
  long best_cost = -1;
  const int nz = (g.ci / 32) * (g.co / 32);
  for (int bpt = 1; bpt <= max_bpt; ++bpt) {                // rounds of 256 resident workgroups x (units per workgroup + the reduction epilogue, ~24 units)
    const long rounds = ((long)tasks * bpt * nz + 255) / 256;
    const long cost = rounds * (ceil_div(nunits, bpt) + 24);
    if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = bpt; }
  }
  upb = ceil_div(ceil_div(nunits, best), 24) * 24;          // whole six-unit trips for each of the four waves (wgrad_bf16.hip)
  blocks = ceil_div(nunits, upb);
}

size_t wgrad_partial_floats(const ConvGeom& g, int tasks) {
  if (use_rows_kernel(g)) {
    int rh, nunits, upb, blocks;
    rows_split(g, tasks, rh, nunits, upb, blocks);
    int nu, ub, bl;                                         // either operand form may be selected at launch time: size for the larger split
    if (wgrad_bf16_ok(g)) {
      rows_split_bf16(g, tasks, nu, ub, bl);
      if (bl > blocks) blocks = bl;
    }
    if (wgrad_bf16_strips(g)) {
      for (int nt = 1; nt <= 2; ++nt) {
        int rw;
        strips_split_bf16(g, tasks, nt, rw, ub, bl);
        if (bl > blocks) blocks = bl;
      }
    }
    return (size_t)tasks * blocks * 9 * g.ci * g.co;
  }
  const int mpix = g.n * g.ho * g.wo;
  const int chunk = wgrad_chunks(mpix, tasks);
  return (size_t)tasks * ceil_div(mpix, chunk) * 9 * g.ci * g.co;
}

static void launch_rows(hipStream_t st, const WgradArgs& a, dim3 grid, int rh, bool exact) {
#define ROWS(R)                                                                                                   \
  do {                                                                                                            \
    if (exact) hipLaunchKernelGGL((wgrad3x3_rows_mfma_kernel<R, true>), grid, dim3(256), 0, st, a);               \
    else hipLaunchKernelGGL((wgrad3x3_rows_mfma_kernel<R, false>), grid, dim3(256), 0, st, a);                    \
  } while (0)
  if (rh == 7) ROWS(7);
  else if (rh == 8) ROWS(8);
  else if (rh == 5) ROWS(5);
  else ROWS(4);
#undef ROWS
}

// Every decision of launch_wgrad3x3 (kernel family, template instance, work split), host arithmetic only: the launcher launches from
// it and mi_debug_wgrad_plan reports it.  have_scales: the fp16 form's largest-magnitude cells are there for every operand.
WgradPlan wgrad_plan(const ConvGeom& g, int tasks, int nterms, bool have_scales) {
  WgradPlan p{};
  p.form = conv_operand_form();
  if (p.form == 2 && !have_scales) p.form = 1;               // no scales: the bf16 form
  const bool split = use_rows_kernel(g) && conv_split_bf16() && (g_conv_split_mask & (1u << (16 + (nterms - 1))));
  if (split && wgrad_bf16_strips(g) && (size_t)g.n * g.h * g.w * g.ci * 4 < (size_t)MI_OOB &&
      !((g_conv_split_mask >> 21) & 1u)) {                     // bit 21 (debug): the unit form on wide maps too
    int rows, ipb, blocks;
    strips_split_bf16(g, tasks, nterms, rows, ipb, blocks);
    p.family = WG_FAM_STRIPS_BF16;
    p.strip_cand = rows;
    p.size = wgrad_bf16_strip_rows(g, rows);
    p.per_block = ipb * nterms;                              // the item stream is nterms x items long, same workgroup count
    p.blocks = p.nchunks = blocks;
    p.per_term = wgrad_bf16_strip_items(g, rows);
    return p;
  }
  if (split && wgrad_bf16_ok(g)) {
    int nunits, upb, blocks;
    rows_split_bf16(g, tasks, nunits, upb, blocks);
    p.family = WG_FAM_ROWS_BF16;
    p.size = 8;
    p.per_block = upb * nterms;                              // the unit stream is nterms x nunits long, same workgroup count
    p.blocks = p.nchunks = blocks;
    p.per_term = nunits;
    return p;
  }
  if (use_rows_kernel(g)) {
    int rh, nunits, upb, blocks;
    rows_split(g, tasks, rh, nunits, upb, blocks);
    p.family = WG_FAM_ROWS_F32;
    p.size = rh;
    // EXACT: segments tile the row exactly and both channel counts are 32 (the 4-conv-32 classifier): immediates instead of per-load adds
    p.exact = g.w % rh == 0 && g.ci == 32 && g.co == 32;
    p.per_block = upb * nterms;                              // the unit stream is nterms x nunits long, same workgroup count
    p.blocks = p.nchunks = blocks;
    p.per_term = nunits;
    return p;
  }
  const int mpix = g.n * g.ho * g.wo;
  p.size = wgrad_chunks(mpix, tasks);
  p.nchunks = ceil_div(mpix, p.size);
  p.per_block = 4;                                           // one chunk per wave
  p.blocks = ceil_div(p.nchunks, 4);
  p.per_term = mpix;
  if (g.ci == 1 || g.ci == 3) p.family = nterms == 1 ? WG_FAM_FIRST : -1;
  else p.family = (g.ci % 32 || g.co % 32) ? -1 : WG_FAM_CHUNKED;
  return p;
}

hipError_t launch_wgrad3x3(hipStream_t st, WgradArgs a, int tasks, int nterms, int* nchunks_out) {
  const int s = a.g.stride;
  const WgradPlan p = wgrad_plan(a.g, tasks, nterms, a.amax_x[0] && a.amax_dz[0] && (nterms == 1 || (a.amax_x[1] && a.amax_dz[1])));
  a.form = p.form;
  a.nchunks = p.nchunks;
  *nchunks_out = p.nchunks;
  if (p.family < 0) return hipErrorInvalidValue;
  const dim3 grid(p.blocks, tasks, p.family == WG_FAM_FIRST ? a.g.co / 32 : (a.g.ci / 32) * (a.g.co / 32));
  if (p.family == WG_FAM_FIRST || p.family == WG_FAM_CHUNKED) {
    a.chunk_pix = p.size;
    if (p.family == WG_FAM_CHUNKED) {
      if (nterms == 1) hipLaunchKernelGGL((wgrad3x3_mfma_kernel<1, 2>), grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL((wgrad3x3_mfma_kernel<2, 2>), grid, dim3(256), 0, st, a);
    } else if (a.g.ci == 3 && s == 1) hipLaunchKernelGGL((wgrad3x3_first_mfma_kernel<3, 1>), grid, dim3(256), 0, st, a);
    else if (a.g.ci == 3 && s == 2) hipLaunchKernelGGL((wgrad3x3_first_mfma_kernel<3, 2>), grid, dim3(256), 0, st, a);
    else if (a.g.ci == 1 && s == 1) hipLaunchKernelGGL((wgrad3x3_first_mfma_kernel<1, 1>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((wgrad3x3_first_mfma_kernel<1, 2>), grid, dim3(256), 0, st, a);
    return hipGetLastError();
  }
  a.nterms = nterms;
  a.chunk_pix = p.per_block;
  if (p.family == WG_FAM_STRIPS_BF16) return launch_wgrad_strips_bf16(st, a, grid, p.strip_cand);
  if (p.family == WG_FAM_ROWS_BF16) return launch_wgrad_rows_bf16(st, a, grid);
  launch_rows(st, a, grid, p.size, p.exact != 0);
  return hipGetLastError();
}

// dW[task] = sum over chunks of the wgrad partials, written at out + task*ostride (tap-major [9][ci][co]).
hipError_t launch_wgrad_reduce(hipStream_t st, const float* partial, int nchunks, int nelem, int tasks, float* out,
                               size_t ostride) {
  const int S = fold_slices(nchunks);
  hipLaunchKernelGGL(reduce_partials_kernel, dim3(ceil_div(nelem, 256 / S), tasks), dim3(256), 0, st, partial, nchunks, nelem, out,
                     ostride, S);
  return hipGetLastError();
}

extern "C" int mi_debug_conv_stamps(void* buf) {
  unsigned long long* p = reinterpret_cast<unsigned long long*>(buf);
  return hipMemcpyToSymbol(HIP_SYMBOL(g_conv_stamps), &p, sizeof(p)) == hipSuccess ? 0 : -2;
}
