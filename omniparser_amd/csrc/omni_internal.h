// Internal helpers shared by the gfx950 kernels of libomni_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include "../../include/omni_amd.h"

void omni_set_error(const char* fmt, ...);

#define OMNI_HIP_CHECK(expr)                                                        \
  do {                                                                              \
    hipError_t _e = (expr);                                                         \
    if (_e != hipSuccess) {                                                         \
      omni_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
      return OMNI_E_HIP;                                                            \
    }                                                                               \
  } while (0)

#define OMNI_REQUIRE(cond, ...)                 \
  do {                                          \
    if (!(cond)) {                              \
      omni_set_error(__VA_ARGS__);              \
      return OMNI_E_ARG;                        \
    }                                           \
  } while (0)

// counted wait on outstanding vector-memory operations (LDS-DMA pieces); the host emulation of tests/emu defines its own
#ifndef OMNI_WAIT_VMCNT
#define OMNI_WAIT_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#endif

// this wave's LDS reads have returned (placed in front of a barrier that releases the buffer they read to other waves' LDS-DMA)
#ifndef OMNI_WAIT_LGKM0
#define OMNI_WAIT_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
#endif

// dynamically sized LDS array of a kernel (size = the launch's shared-memory argument)
#ifndef OMNI_DYN_LDS
#define OMNI_DYN_LDS(type, name) extern __shared__ type name[]
#endif

// lanes of ONE wave exchange data through LDS (write, OMNI_WAVE_SYNC, read): the hardware executes a wave's LDS instructions in
// order, so only the compiler must be kept from reordering (a build that runs work-items as fibers defines its own rendezvous)
#ifndef OMNI_WAVE_SYNC
#define OMNI_WAVE_SYNC() __builtin_amdgcn_wave_barrier()
#endif

typedef _Float16 half_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <typename T> struct ElemTraits;
template <> struct ElemTraits<float> {
  static constexpr int kVec = 4;   // elements per 16-byte vector
  static __host__ __device__ __forceinline__ float to_f32(float v) { return v; }
  static __host__ __device__ __forceinline__ float from_f32(float v) { return v; }
};
template <> struct ElemTraits<half_t> {
  static constexpr int kVec = 8;
  static __host__ __device__ __forceinline__ float to_f32(half_t v) { return (float)v; }
  static __host__ __device__ __forceinline__ half_t from_f32(float v) { return (half_t)v; }
};

// ---- range guard of the split formats (round 6).  Both split formats hold their hi half in f16, so |x| > 65504 cannot be represented:
// format B clamps (below), format A (conv_igemm.hip::split_f16x4) would convert to the largest finite half and lose the value.  The
// reference computes in fp32 and has no such limit (ref:util/utils.py:66), and the stand-in checkpoints never come near it — a real
// checkpoint that does must not diverge silently.  Every kernel that writes a split tensor, and every convolution epilogue whose f32
// output a format-A loader will split, tracks max |x| of what it produced and bumps a per-translation-unit device counter when that
// exceeds the f16 range: omni_split4(v, hi, lo) reports by itself (HBM-bound producers), the accumulating form (..., amax) +
// omni_report_range(amax) costs two v_max3_f32 per four values and one compare per thread (the GEMM epilogues).  The host sums the
// counters with omni_overflow_count() (include/omni_amd.h); `ScreenParser` reads it once per batch into stats["split_overflow"] and
// raises when OMNI_STRICT_RANGE=1 (parity runs).
static __device__ unsigned int omni_ovf_count_tu;
#define OMNI_F16_MAX 65504.0f
__device__ __forceinline__ float omni_amax4(const float* v, float amax) {
  amax = __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[0]), __builtin_fabsf(v[1])), amax);
  return __builtin_fmaxf(__builtin_fmaxf(__builtin_fabsf(v[2]), __builtin_fabsf(v[3])), amax);
}
__device__ __forceinline__ void omni_report_range(float amax) {
  if (__builtin_expect(amax > OMNI_F16_MAX, 0)) atomicAdd(&omni_ovf_count_tu, 1u);
}
// host side, once per translation unit that contains such kernels: registers a reader of this unit's counter with capi.hip
typedef int (*omni_ovf_reader_t)(unsigned int* count, int reset);
void omni_register_overflow_reader(omni_ovf_reader_t fn);
#define OMNI_RANGE_GUARD_TU()                                                                                               \
  namespace {                                                                                                               \
  int omni_ovf_read_tu(unsigned int* count, int reset) {                                                                    \
    unsigned int v = 0;                                                                                                     \
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(omni_ovf_count_tu), sizeof v, 0, hipMemcpyDeviceToHost) != hipSuccess) return 1; \
    if (reset && v) {                                                                                                       \
      const unsigned int z = 0;                                                                                             \
      if (hipMemcpyToSymbol(HIP_SYMBOL(omni_ovf_count_tu), &z, sizeof z, 0, hipMemcpyHostToDevice) != hipSuccess) return 1; \
    }                                                                                                                       \
    *count = v;                                                                                                             \
    return 0;                                                                                                               \
  }                                                                                                                         \
  struct OmniOvfReg { OmniOvfReg() { omni_register_overflow_reader(&omni_ovf_read_tu); } } omni_ovf_reg;                   \
  }

// "Format B" split of 4 consecutive channels: x = hi + lo, hi = f16(x) (rtz), lo = f16(x - hi), |x| clamped to the f16 range (and
// counted by the range guard above when the clamp bites).
// A 16-channel group occupies 64 bytes: 16 hi halves then 16 lo halves (gemm_dma.hip consumes it by LDS-DMA).
__device__ __forceinline__ void omni_split4_raw(const float* v, uint2& hi, uint2& lo) {
  typedef __fp16 hv2 __attribute__((ext_vector_type(2)));
  float c[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) c[e] = __builtin_fminf(__builtin_fmaxf(v[e], -OMNI_F16_MAX), OMNI_F16_MAX);
  hv2 h01 = __builtin_amdgcn_cvt_pkrtz(c[0], c[1]);
  hv2 h23 = __builtin_amdgcn_cvt_pkrtz(c[2], c[3]);
  // x - hi is exact in f32 (hi is x truncated to 11 significant bits), so the fused form gives the same bits as convert + subtract; it
  // compiles to one mixed-precision fma that reads the half directly
  float m1 = -1.0f;
  asm("" : "+r"(m1));                             // opaque to the optimiser, which would turn fma(h, -1, x) back into convert + subtract
  hv2 l01 = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)h01[0], m1, c[0]), __builtin_fmaf((float)h01[1], m1, c[1]));
  hv2 l23 = __builtin_amdgcn_cvt_pkrtz(__builtin_fmaf((float)h23[0], m1, c[2]), __builtin_fmaf((float)h23[1], m1, c[3]));
  hi.x = __builtin_bit_cast(unsigned, h01); hi.y = __builtin_bit_cast(unsigned, h23);
  lo.x = __builtin_bit_cast(unsigned, l01); lo.y = __builtin_bit_cast(unsigned, l23);
}
__device__ __forceinline__ void omni_split4(const float* v, uint2& hi, uint2& lo, float& amax) {   // accumulating: caller reports once
  amax = omni_amax4(v, amax);
  omni_split4_raw(v, hi, lo);
}
__device__ __forceinline__ void omni_split4(const float* v, uint2& hi, uint2& lo) {               // self-reporting
  omni_report_range(omni_amax4(v, 0.0f));
  omni_split4_raw(v, hi, lo);
}
// one value -> (hi, lo) halves, and its place in a split row of halves: element index of the hi half (lo = +16 halves)
__device__ __forceinline__ void omni_split1(float v, unsigned short& hi, unsigned short& lo) {
  typedef __fp16 hv2 __attribute__((ext_vector_type(2)));
  omni_report_range(__builtin_fabsf(v));
  v = __builtin_fminf(__builtin_fmaxf(v, -OMNI_F16_MAX), OMNI_F16_MAX);
  hv2 h = __builtin_amdgcn_cvt_pkrtz(v, 0.0f);
  hv2 l = __builtin_amdgcn_cvt_pkrtz(v - (float)h[0], 0.0f);
  hi = (unsigned short)(__builtin_bit_cast(unsigned, h) & 0xffffu);
  lo = (unsigned short)(__builtin_bit_cast(unsigned, l) & 0xffffu);
}
__device__ __forceinline__ int omni_split_half_index(int c) { return (c >> 4) * 32 + (c & 15); }
// byte offset of channel c (c % 4 == 0) inside a split row: hi halves; the lo halves sit 32 bytes further
__device__ __forceinline__ int omni_split_off(int c) { return (c >> 4) * 64 + (c & 15) * 2; }

// erf for the exact GELU of the captioner's FFN epilogues (hf ACT2FN["gelu"]: 0.5 x (1 + erf(x / sqrt 2))).  ocml's erff inlines to
// ~55 instructions per element (7 800 of the 9 900 instructions of the 256x256 GELU GEMM kernel; its epilogue cost a third of a K = 512
// layer's time and all of a K = 128 layer's).  This one is branch-free, division-free, ~25 instructions: two minimax
// polynomials (|x| <= 0.9277: odd polynomial in x; above: 1 - exp(p(|x|))), both evaluated, one select.  Maximum error 0.99 ulp /
// 5.9e-8 absolute against a float64 erf over [-6, 6] and N(0, 1.5) samples (tests/test_host_cpu.py::test_erf_polynomial restates it
// in numpy); |x| is clamped to 6 (erf = 1 in f32 from 3.92 on) so that no inf - inf can appear.
__device__ __forceinline__ float omni_erff(float a) {
  const float t = __builtin_fminf(__builtin_fabsf(a), 6.0f), s = t * t;
  float r = __builtin_fmaf(-1.72853470e-5f, t, 3.83197126e-4f);
  const float u = __builtin_fmaf(-3.88396438e-3f, t, 2.42546219e-2f);
  r = __builtin_fmaf(r, s, u);
  r = __builtin_fmaf(r, t, -1.06777847e-1f);
  r = __builtin_fmaf(r, t, -6.34846687e-1f);
  r = __builtin_fmaf(r, t, -1.28717512e-1f);
  r = __builtin_fmaf(r, t, -t);
  const float big = __builtin_copysignf(1.0f - __expf(r), a);
  float q = -5.96761703e-4f;
  q = __builtin_fmaf(q, s, 4.99119423e-3f);
  q = __builtin_fmaf(q, s, -2.67681349e-2f);
  q = __builtin_fmaf(q, s, 1.12819925e-1f);
  q = __builtin_fmaf(q, s, -3.76125336e-1f);
  q = __builtin_fmaf(q, s, 1.28379166e-1f);
  const float small = __builtin_fmaf(q, a, a);
  return t > 0.927734375f ? big : small;
}
__device__ __forceinline__ float omni_gelu(float v) { return 0.5f * v * (1.0f + omni_erff(v * 0.70710678118654752440f)); }
// GELU of the GEMM epilogues, two elements per packed v_pk_*_f32 instruction (full rate on gfx950).  Those epilogues run with the
// matrix pipe idle, so every instruction here is wall time; this form evaluates ONE polynomial and no select:
//   t = min(|v|, 6 sqrt 2),  E = exp2(p(t)) ~ erfc(t / sqrt 2),  1 + erf(v / sqrt 2) = E for v < 0 and 2 - E otherwise, so
//   gelu(v) = v * (c0 - c1 * E)  with  c1 = copysign(0.5, v),  c0 = 0.5 + c1  (1 or 0).
// For v < 0 nothing cancels (the two-polynomial omni_gelu above returns 0 below v = -5.6 and loses digits from v = -1 on); for v > 0
// an absolute error of E is a relative error of the same size in the result.  p is a degree-11 weighted minimax fit of
// log2 erfc(|v| / sqrt 2) on [0, 6 sqrt 2] (log2 e and 1 / sqrt 2 folded in; tools/fit_gelu_erfc.py: Lawson iteration in float64, error
// of E 1.3e-8).  Evaluated in f32 Horner form as below, against a float64 GELU on the samples of tests/test_gelu_onebranch_cpu.py:
// max abs 3.84e-7, max rel 5.5e-4 where the reference is a normal number (omni_gelu: 4.47e-7, 1.0).  21 instructions per pair with the
// bias fma of the caller (tools/gemm_epilogue_isa.py), 33 for the packed two-polynomial form it replaced.
// The halving of 0.5 * v * (1 + erf) sits in c0 / c1: halving commutes with rounding outside the subnormal range, so v * fma(0.5, e, 0.5)
// already had the bits of (0.5 * v) * (1 + e) for the two-polynomial e (compared bitwise in the same test).
typedef float f32x2 __attribute__((ext_vector_type(2)));
#if defined(__AMDGCN__)
#define OMNI_EXP2(x) __builtin_amdgcn_exp2f(x)     // bare v_exp_f32: the argument is in [-56, 0]
#else
#define OMNI_EXP2(x) __builtin_exp2f(x)
#endif
__device__ __forceinline__ f32x2 omni_gelu2(f32x2 v) {
  const f32x2 t = __builtin_elementwise_min(__builtin_elementwise_abs(v), (f32x2)8.48528137423857f);
  f32x2 p = __builtin_elementwise_fma((f32x2)1.137868688e-09f, t, (f32x2)-5.171069262e-08f);
  p = __builtin_elementwise_fma(p, t, (f32x2)1.014483701e-06f);
  p = __builtin_elementwise_fma(p, t, (f32x2)-1.117507963e-05f);
  p = __builtin_elementwise_fma(p, t, (f32x2)7.388171798e-05f);
  p = __builtin_elementwise_fma(p, t, (f32x2)-2.645340865e-04f);
  p = __builtin_elementwise_fma(p, t, (f32x2)-3.723767077e-05f);
  p = __builtin_elementwise_fma(p, t, (f32x2)6.994847674e-03f);
  p = __builtin_elementwise_fma(p, t, (f32x2)-5.247364566e-02f);
  p = __builtin_elementwise_fma(p, t, (f32x2)-4.592104554e-01f);
  p = __builtin_elementwise_fma(p, t, (f32x2)-1.151105404e+00f);
  p = __builtin_elementwise_fma(p, t, (f32x2)1.941864447e-08f);
  const f32x2 E = {OMNI_EXP2(p[0]), OMNI_EXP2(p[1])};
  const f32x2 c1 = __builtin_elementwise_copysign((f32x2)0.5f, v);
  return v * __builtin_elementwise_fma(-c1, E, 0.5f + c1);
}

// per-kind launchers (each lives in its own .hip file)
int omni_launch_conv(const omni_op_t* op, hipStream_t s);
int omni_launch_gemm_dma(const omni_op_t* op, hipStream_t s);
int omni_launch_split_convert(const omni_op_t* op, hipStream_t s);
int omni_launch_chan_repack(const omni_op_t* op, hipStream_t s);   // OMNI_OP_SPLIT_CONVERT i6 = 1
int omni_launch_mlp_fused(const omni_op_t* op, hipStream_t s);
int omni_launch_avgpool2(const omni_op_t* op, hipStream_t s);
int omni_launch_maxpool(const omni_op_t* op, hipStream_t s);
int omni_launch_resize_nearest(const omni_op_t* op, hipStream_t s);
int omni_launch_letterbox(const omni_op_t* op, hipStream_t s);
int omni_launch_detect_decode(const omni_op_t* op, hipStream_t s);
int omni_launch_nms(const omni_op_t* op, hipStream_t s);
int omni_launch_dwconv3(const omni_op_t* op, hipStream_t s);
int omni_launch_layernorm(const omni_op_t* op, hipStream_t s);
int omni_launch_dwconv3_ln(const omni_op_t* op, hipStream_t s);
int omni_launch_attention(const omni_op_t* op, hipStream_t s);
int omni_launch_misc(const omni_op_t* op, hipStream_t s);
int omni_launch_vocab_step(const omni_op_t* op, hipStream_t s);
int omni_launch_visual_match(const omni_op_t* op, hipStream_t s);
long long omni_visual_match_part_bytes(const omni_op_t* op);
int omni_launch_region_ocr(const omni_op_t* op, hipStream_t s);
bool omni_region_ocr_extents(const omni_op_t* op, long long ext[8]);
int omni_launch_glue(const omni_op_t* op, hipStream_t s);
int omni_launch_overlay(const omni_op_t* op, hipStream_t s);
int omni_launch_png_pack(const omni_op_t* op, hipStream_t s);
int omni_launch_png_deflate(const omni_op_t* op, hipStream_t s);
