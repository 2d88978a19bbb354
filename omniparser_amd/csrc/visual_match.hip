// OMNI_OP_VISUAL_MATCH: which element looks like this one?  Row 0 of a crop's img_feat (the spatial-average token behind
// image_projection and image_proj_norm; transformers' get_image_features(...).pooler_output) is Florence-2's own global descriptor of
// the crop.  Three modes (i0), see include/omni_amd.h:
//
//   0 embed     row 0 of every crop of an img_feat tensor -> the L2-normalised vector (f32) and its norm; one wave per crop
//   1 partial   unit queries x unit gallery: a block scores one slice of the gallery against one group of 8 queries (a gallery row
//               is loaded once per group, 16 bytes per lane) and keeps each query's best k -> partials
//   2 merge     one small launch folds the partials of each query into idx / score (descending score, lower gallery index first
//               among equals, -1 / -inf behind min(k, n)).  A second launch on purpose: DESIGN §7 item 4 measured the in-launch
//               combine as slower at this size.
//
// The score of a pair (q, g) is the plain f32 dot product in ONE summation order that depends on D alone: lane l adds the products
// of elements 4 l + 256 j .. + 3 as (x + y) + (z + w), j ascending, then the 64 lanes are folded by an xor butterfly (32, 16, ..., 1).
// Neither the split, nor the wave that meets the row, nor the query's place in its group enters, so a pair has the same bits in
// every launch geometry (the split override i5 is the test handle for exactly that).
// The helpers below are copies of the few lines of caption_ops.hip / vocab_step.hip (whose kernels keep their machine code).
#include "omni_internal.h"

#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxK = 8, kMaxD = 4096, kMaxM = 4096, kMaxN = 65536;
constexpr int kGroup = 8;                 // queries per block; also the lanes that hold one query's sorted list
constexpr int kLdsQueryFloats = 12288;    // 48 KiB: the query group is staged in LDS up to D = 1536, read through the caches beyond
constexpr int kTargetBlocks = 1024;       // 256 CUs x 4 resident blocks
constexpr int kMinSlice = 256;            // gallery rows per block below which splitting stops paying for the query staging

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <typename T> __device__ __forceinline__ f32x4 load4(const T* p);
template <> __device__ __forceinline__ f32x4 load4<float>(const float* p) { return *(const f32x4*)p; }
template <> __device__ __forceinline__ f32x4 load4<half_t>(const half_t* p) {
  const f16x4 h = *(const f16x4*)p;
  return f32x4{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
}

// ---------------------------------------------------------------------------------------------- mode 0
// One wave per crop, four crops per block.  Sum of squares in f32 ((x2 + y2) + (z2 + w2) per 16-byte load, then the butterfly), one
// correctly rounded square root, one correctly rounded division per element; a zero row divides nothing.
template <typename T>
__global__ __launch_bounds__(256) void embed_rows_kernel(const T* x, float* y, float* norm, int n, long long ld, int D) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n) return;                    // the whole wave leaves
  const T* xr = x + row * ld;
  float ss = 0.0f;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = load4(xr + c);
    ss += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
  }
  ss = wave_sum(ss);
  const float nm = sqrtf(ss);
  float* yr = y + (long long)row * D;
  for (int c = lane * 4; c < D; c += 256) {
    const f32x4 v = load4(xr + c);          // 3 KB per crop at D = 768: from the L1 it was just read through
    *(f32x4*)(yr + c) = nm > 0.0f ? f32x4{v.x / nm, v.y / nm, v.z / nm, v.w / nm} : f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  if (lane == 0) norm[row] = nm;
}

// ---------------------------------------------------------------------------------------------- modes 1 and 2
struct Entry { float s; int i; };          // a partial: score and gallery index (-inf / -1 = empty)

struct MatchArgs {
  const float* q; const float* g; Entry* part; int* idx; float* score;
  int m, n, D, k, len, S;
};

// c comes before e: the larger score, the lower gallery index among equals; an empty entry (-1, compared unsigned) comes last.
// A NaN score comes before nothing and is never kept.
__device__ __forceinline__ bool before(float cs, int ci, float es, int ei) {
  return cs > es || (cs == es && (unsigned)ci < (unsigned)ei);
}

// The sorted list of a query lies across the 8 lanes of its lane group: lane & 7 is the rank, (s, i) the entry.  Insert the candidate
// (the same in all 8 lanes): ranks in front of its place keep their entry, its place takes it, ranks behind take their neighbour's.
__device__ __forceinline__ void insert(float& s, int& i, float cs, int ci, int lane) {
  const int src = (lane & ~7) | ((lane - 1) & 7);
  const float ps = __shfl(s, src);
  const int pi = __shfl(i, src);
  if (before(cs, ci, s, i)) {
    const bool shift = (lane & 7) != 0 && before(cs, ci, ps, pi);
    s = shift ? ps : cs;
    i = shift ? pi : ci;
  }
}

// grid (splits, query groups), 4 waves.  Wave w takes rows w, w + 4, ... of the block's slice; a lane holds 8 accumulators, one per
// query of the group.  The 8 wave sums are folded TRANSPOSED: at offsets 32, 16 and 8 a lane keeps half of its values and hands the
// other half to its partner (4 + 2 + 1 exchanges), then three plain butterfly steps — 10 exchanges instead of 48, and since a + b is
// b + a every lane ends with the bits the plain butterfly gives: lane l holds the score of query l >> 3, eight copies per query,
// which is where that query's sorted list lives (rank l & 7).
template <bool LDSQ>
__global__ __launch_bounds__(256) void match_partial_kernel(MatchArgs a) {
  OMNI_DYN_LDS(f32x4, lds);                // LDSQ: the query group [8][D / 4]; then Entry [4 waves][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x, q0 = blockIdx.y * kGroup, nq = min(kGroup, a.m - q0);
  const int D4 = a.D >> 2;
  // a group's rows beyond the last query repeat it: computed, never written
  if constexpr (LDSQ) {
    for (int e = tid; e < kGroup * D4; e += 256) {
      const int qi = min(q0 + e / D4, a.m - 1);
      lds[e] = ((const f32x4*)(a.q + (long long)qi * a.D))[e % D4];
    }
    __syncthreads();
  }
  const f32x4* qrow[kGroup];
#pragma unroll
  for (int qi = 0; qi < kGroup; ++qi)
    qrow[qi] = LDSQ ? lds + qi * D4 : (const f32x4*)(a.q + (long long)min(q0 + qi, a.m - 1) * a.D);
  Entry* ent = (Entry*)(lds + (LDSQ ? kGroup * D4 : 0));
  const int g_end = min(a.n, (split + 1) * a.len);
  const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
  float ls = -INFINITY;
  int li = -1;
  for (int g = split * a.len + wave; g < g_end; g += 4) {      // ascending per wave: among equal scores the earlier row stays in front
    const f32x4* gr = (const f32x4*)(a.g + (long long)g * a.D);
    float acc[kGroup];
#pragma unroll
    for (int qi = 0; qi < kGroup; ++qi) acc[qi] = 0.0f;
    for (int c = lane; c < D4; c += 64) {
      const f32x4 gv = gr[c];
#pragma unroll
      for (int qi = 0; qi < kGroup; ++qi) {
        const f32x4 qv = qrow[qi][c];
        acc[qi] += (gv.x * qv.x + gv.y * qv.y) + (gv.z * qv.z + gv.w * qv.w);
      }
    }
    float r4[4], r2[2];
#pragma unroll
    for (int t = 0; t < 4; ++t) r4[t] = (h5 ? acc[t + 4] : acc[t]) + __shfl_xor(h5 ? acc[t] : acc[t + 4], 32);
#pragma unroll
    for (int t = 0; t < 2; ++t) r2[t] = (h4 ? r4[t + 2] : r4[t]) + __shfl_xor(h4 ? r4[t] : r4[t + 2], 16);
    float r = (h3 ? r2[1] : r2[0]) + __shfl_xor(h3 ? r2[0] : r2[1], 8);
    r += __shfl_xor(r, 4);
    r += __shfl_xor(r, 2);
    r += __shfl_xor(r, 1);
    insert(ls, li, r, g, lane);
  }
  ent[wave * 64 + lane] = Entry{ls, li};
  __syncthreads();
  if (wave != 0) return;
  for (int w = 1; w < 4; ++w)
    for (int rnk = 0; rnk < kGroup; ++rnk) {
      const Entry c = ent[w * 64 + (lane & ~7) + rnk];
      insert(ls, li, c.s, c.i, lane);
    }
  const int qi = lane >> 3, rnk = lane & 7;
  if (qi < nq && rnk < a.k) a.part[((long long)(q0 + qi) * a.S + split) * a.k + rnk] = Entry{ls, li};
}

// one wave per 8 queries: every lane group walks the S x k partials of its query in order
__global__ __launch_bounds__(64) void match_merge_kernel(MatchArgs a) {
  const int lane = threadIdx.x, q = blockIdx.x * kGroup + (lane >> 3), rnk = lane & 7;
  const Entry* p = a.part + (long long)min(q, a.m - 1) * a.S * a.k;
  float ls = -INFINITY;
  int li = -1;
  const int cnt = a.S * a.k;
  for (int e = 0; e < cnt; ++e) {
    const Entry c = p[e];
    insert(ls, li, c.s, c.i, lane);
  }
  if (q < a.m && rnk < a.k) {
    a.idx[(long long)q * a.k + rnk] = li;
    a.score[(long long)q * a.k + rnk] = ls;
  }
}

// the i-slots of modes 1 and 2 -> the launch geometry, validated; no pointer is looked at
int match_cfg(const omni_op_t* op, MatchArgs& a) {
  a.m = op->i[1]; a.n = op->i[2]; a.D = op->i[3]; a.k = op->i[4];
  OMNI_REQUIRE(a.m >= 1 && a.m <= kMaxM, "visual_match: %d queries (i1), 1..%d", a.m, kMaxM);
  OMNI_REQUIRE(a.n >= 1 && a.n <= kMaxN, "visual_match: a gallery of %d rows (i2), 1..%d", a.n, kMaxN);
  OMNI_REQUIRE(a.D >= 4 && a.D <= kMaxD && a.D % 4 == 0, "visual_match: D = %d (i3), a multiple of 4 up to %d", a.D, kMaxD);
  OMNI_REQUIRE(a.k >= 1 && a.k <= kMaxK, "visual_match: k = %d (i4), 1..%d", a.k, kMaxK);
  OMNI_REQUIRE(op->i[5] >= 0, "visual_match: split length %d (i5), 0 = the launcher's choice", op->i[5]);
  if (op->i[5] > 0) {
    a.len = op->i[5];
  } else {
    const int groups = (a.m + kGroup - 1) / kGroup;
    const int splits = min(max(1, kTargetBlocks / groups), max(1, a.n / kMinSlice));
    a.len = ((a.n + splits - 1) / splits + 3) & ~3;        // whole rounds of the block's 4 waves
  }
  a.S = (a.n + a.len - 1) / a.len;
  return OMNI_OK;
}

long long part_bytes(const MatchArgs& a) { return (long long)a.m * a.S * a.k * (long long)sizeof(Entry); }

int launch_embed(const omni_op_t* op, hipStream_t s) {
  const int n = op->i[1], D = op->i[3];
  const long long ld = op->i[2];
  OMNI_REQUIRE(n >= 1 && n <= kMaxN, "visual_match embed: %d crops (i1), 1..%d", n, kMaxN);
  OMNI_REQUIRE(D >= 4 && D <= kMaxD && D % 4 == 0, "visual_match embed: D = %d (i3), a multiple of 4 up to %d", D, kMaxD);
  OMNI_REQUIRE(ld >= D && ld % 4 == 0, "visual_match embed: row stride %lld (i2), a multiple of 4 of at least D = %d", ld, D);
  OMNI_REQUIRE(op->dtype == OMNI_F32 || op->dtype == OMNI_F16, "visual_match embed: unsupported dtype %d", op->dtype);
  OMNI_REQUIRE(op->p[0] && op->p[4] && op->p[5], "visual_match embed: p0 (img_feat), p4 (vectors) or p5 (norms) is NULL");
  OMNI_REQUIRE((unsigned long long)op->p[0] % (op->dtype == OMNI_F32 ? 16 : 8) == 0 && (unsigned long long)op->p[4] % 16 == 0 &&
               (unsigned long long)op->p[5] % 4 == 0, "visual_match embed: p0 / p4 not aligned to 4 elements, or p5 not to 4 bytes");
  const dim3 grid((n + 3) / 4);
  if (op->dtype == OMNI_F32)
    hipLaunchKernelGGL((embed_rows_kernel<float>), grid, dim3(256), 0, s, (const float*)op->p[0], (float*)op->p[4], (float*)op->p[5], n, ld, D);
  else
    hipLaunchKernelGGL((embed_rows_kernel<half_t>), grid, dim3(256), 0, s, (const half_t*)op->p[0], (float*)op->p[4], (float*)op->p[5], n, ld, D);
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}

}  // namespace

// bytes of the partials buffer (p5) modes 1 and 2 touch; 0 for an op whose slots the launcher refuses (capi.hip::op_extents)
long long omni_visual_match_part_bytes(const omni_op_t* op) {
  MatchArgs a{};
  return match_cfg(op, a) == OMNI_OK ? part_bytes(a) : 0;
}

extern "C" int omni_visual_match_cfg(const omni_op_t* op, long long out[4]) {
  OMNI_REQUIRE(op && out, "omni_visual_match_cfg: null argument");
  OMNI_REQUIRE(op->kind == OMNI_OP_VISUAL_MATCH && (op->i[0] == 1 || op->i[0] == 2), "omni_visual_match_cfg: not a mode 1 / 2 visual_match op");
  MatchArgs a{};
  if (int rc = match_cfg(op, a)) return rc;
  out[0] = (a.m + kGroup - 1) / kGroup; out[1] = a.len; out[2] = a.S; out[3] = part_bytes(a);
  return OMNI_OK;
}

int omni_launch_visual_match(const omni_op_t* op, hipStream_t s) {
  const int mode = op->i[0];
  if (mode == 0) return launch_embed(op, s);
  OMNI_REQUIRE(mode == 1 || mode == 2, "visual_match: mode %d (i0), 0 = embed, 1 = partial top-k, 2 = merge", mode);
  MatchArgs a{};
  if (int rc = match_cfg(op, a)) return rc;
  a.q = (const float*)op->p[0]; a.g = (const float*)op->p[1]; a.part = (Entry*)op->p[5];
  a.idx = (int*)op->p[4]; a.score = (float*)op->p[6];
  OMNI_REQUIRE(a.part && (unsigned long long)a.part % 8 == 0, "visual_match: p5 (partials) is NULL or not 8-byte aligned");
  OMNI_REQUIRE((long long)op->i[6] >= part_bytes(a), "visual_match: a partials buffer of %d bytes (i6) for %d queries x %d splits of %d rows x k = %d "
               "needs %lld", op->i[6], a.m, a.S, a.len, a.k, part_bytes(a));
  if (mode == 1) {
    OMNI_REQUIRE(a.q && a.g, "visual_match: p0 (queries) or p1 (gallery) is NULL");
    OMNI_REQUIRE((unsigned long long)a.q % 16 == 0 && (unsigned long long)a.g % 16 == 0, "visual_match: p0 / p1 not 16-byte aligned");
    const bool ldsq = kGroup * a.D <= kLdsQueryFloats;
    const size_t lds = (ldsq ? (size_t)kGroup * a.D * 4 : 0) + 4 * 64 * sizeof(Entry);
    const dim3 grid(a.S, (a.m + kGroup - 1) / kGroup);
    if (ldsq) hipLaunchKernelGGL((match_partial_kernel<true>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((match_partial_kernel<false>), grid, dim3(256), lds, s, a);
  } else {
    OMNI_REQUIRE(a.idx && a.score, "visual_match: p4 (idx) or p6 (score) is NULL");
    OMNI_REQUIRE((unsigned long long)a.idx % 4 == 0 && (unsigned long long)a.score % 4 == 0, "visual_match: p4 / p6 not 4-byte aligned");
    hipLaunchKernelGGL(match_merge_kernel, dim3((a.m + kGroup - 1) / kGroup), dim3(64), 0, s, a);
  }
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}
