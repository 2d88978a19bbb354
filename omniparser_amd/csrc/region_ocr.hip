// OMNI_OP_REGION_OCR: Florence-2's <OCR_WITH_REGION> task and its box-answer tasks over native-resolution tiles of a screenshot.
// Five modes (i0), see include/omni_amd.h:
//
//   0 tile cut      n windows of R x R pixels of the HBM-resident u8 [H, W, 3] frame, at origins read from a device table, rescaled
//                   and normalised into a caption plan's input exactly as the image processor does without its resize; a pixel
//                   outside the frame is white (u8 255) before normalisation.  One work-item per tile pixel.
//   1 region parse  one 64-lane block per row of generated ids: the answer "text <loc>x8 text <loc>x8 ..." is cut into regions,
//                   the location bins are de-quantised to frame pixels, every region gets the sum of its tokens'
//                   log-probabilities and a flag saying whether its own tile owns it.  Token classes come from a table in device
//                   memory, so the kernel knows no tokenizer.
//   3 box parse     the same block per row for the answers of the grounding / detection tasks, "phrase <loc>x4 <loc>x4 phrase
//                   <loc>x4 ...": every box gets its corners in frame pixels, the columns of its phrase, the two sums of
//                   log-probabilities (phrase, the box's four location tokens) and the ownership flag.
//   5 polygon parse the same block per row for the answers of the two segmentation tasks, "<loc>x2k <sep> <loc>x2k ..." with or
//                   without <poly> ... </poly> around an instance: every polygon gets its vertices in frame pixels, its columns, the
//                   sum of its vertex tokens' log-probabilities, and its instance's bounding box and ownership flag.
//   6 mask raster   mode 5's records, row counters and vertices, read where mode 5 left them, become one tile-local bit mask per
//                   instance and the number of set pixels per pixel row.  One wave per pixel row.
// (2 and 4 are refused: the tests of modes 1 and 3 launch them with those modes' arguments and expect OMNI_E_ARG.)
//
// Mode 1 works on the row with its STRIP tokens taken out, which is what transformers does to the decoded text before it applies its
// pattern `(.+?)(<loc_n>){8}`: from p = 0, e is the smallest index >= p + 1 whose eight tokens e .. e + 7 are all location tokens; the
// region's content is [p, e), then p = e + 8.  The walk is a dependent chain, so lane 0 makes it over the classes staged in LDS
// (every lane classifies and stages them first); the regions it finds are then finished one lane per region, each with a plain
// sequential f32 sum in ascending token order — the bits do not depend on the launch geometry, and a host twin repeats them.
// Column 0 of a row is the decoder start token and never part of the answer; the row ends in front of the first EOS behind it, and
// nothing behind that EOS reaches an output.
//
// Mode 3 restates transformers' two patterns on the same stripped row, cut into alternating maximal runs of text and location tokens:
// `[^<]+(?:<loc_n>){4,}` (grammar 0) takes a text run and ALL location tokens behind it when there are four or more, and a box per
// four of them; where fewer follow, the pattern's next chance starts INSIDE the run's last `<loc_n>` (behind its '<'), so that token
// leads the next phrase (`lead`: its text counts without the first character); a row that begins with five or more location tokens
// gives its first one as such a phrase.  `(?:<loc_n>){4,}` (grammar 1) takes every run of four or more, without a phrase.
//
// Mode 5 restates parse_description_with_polygons_from_text_and_spans(allow_empty_phrase = True) on the stripped row.  With the location
// bins, <sep>, <poly> and </poly> as STRUCTURE tokens, `(?:<loc_n>|<sep>|<poly>|</poly>){4,}` takes every maximal run of four or more of
// them; a run counts when a location token or <poly> stands behind its first token or, if that is no location token, anywhere in it
// (the phrase pattern's look-ahead).  A run with both <poly> and </poly> is cut into the `<poly>(.*?)</poly>` pairs, left to right;
// any other run is one instance.  Inside an instance `((?:<loc_n>)+)(?:<sep>|$)` makes a polygon of every maximal sequence of location
// tokens that <sep> or the instance's end follows.  Lane 0 walks, one lane per polygon finishes; the bounding box of an instance is
// folded by the lane of its first polygon over the boxes the others left in LDS.
//
// Mode 6 is exact: a pixel's centre (2x + 1, 2y + 1) against vertices 2v in 64-bit integers, even-odd per polygon, so a centre is never
// on an edge's end row and never needs a tie rule.  The instance's vertices are staged in LDS once per block of four pixel rows; each
// lane owns one pixel of a 64-pixel span and the two mask words of the span come from an OR over each half-wave.
#include "omni_internal.h"

#include <limits.h>

#pragma clang fp contract(off)

namespace {

constexpr int kMaxTiles = 65536, kMaxR = 65536, kMaxT = 2049, kMaxM = (kMaxT - 1) / 9, kMaxB = (kMaxT - 1) / 4;
constexpr int kStrip = OMNI_OCR_CLASS_STRIP, kHard = OMNI_OCR_CLASS_HARD;      // 0..999: the location bin itself
constexpr int kSep = OMNI_OCR_CLASS_SEP, kPoly = OMNI_OCR_CLASS_POLY, kPolyEnd = OMNI_OCR_CLASS_POLY_END;   // mode 5 alone
constexpr int kMaxP = kMaxT / 2, kMaxV = (kMaxT - 1) / 2, kMaxI = 64;         // polygon and vertex slots of a row, instance slots of mode 6

// ---------------------------------------------------------------------------------------------- mode 0
struct CutArgs {
  const unsigned char* img; const int* origins; void* y; const float* lut;
  int n, H, W, R, ldo; float mean[3], stdv[3];
};

template <typename T>
__global__ __launch_bounds__(256) void tile_cut_kernel(CutArgs a) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const int tile = blockIdx.y;
  if (idx >= (long long)a.R * a.R) return;
  const int yy = (int)(idx / a.R), xx = (int)(idx - (long long)yy * a.R);
  const long long sx = (long long)a.origins[tile * 2] + xx, sy = (long long)a.origins[tile * 2 + 1] + yy;
  int p[3] = {255, 255, 255};                                // outside the frame: the white canvas the tile is pasted on
  if (sx >= 0 && sx < a.W && sy >= 0 && sy < a.H) {
    const unsigned char* s = a.img + (sy * a.W + sx) * 3;
    p[0] = s[0]; p[1] = s[1]; p[2] = s[2];
  }
  T* out = (T*)a.y + ((long long)tile * a.R * a.R + idx) * a.ldo;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float v = a.lut[p[c]];                             // f32(f64(p) * (1/255)), the table OMNI_OP_CROP_RESIZE reads
    out[c] = ElemTraits<T>::from_f32((v - a.mean[c]) / a.stdv[c]);
  }
  for (int c = 3; c < a.ldo; ++c) out[c] = ElemTraits<T>::from_f32(0.0f);
}

int launch_cut(const omni_op_t* op, hipStream_t s) {
  CutArgs a{};
  a.img = (const unsigned char*)op->p[0]; a.origins = (const int*)op->p[1]; a.y = op->p[4]; a.lut = (const float*)op->p[7];
  a.n = op->i[1]; a.H = op->i[2]; a.W = op->i[3]; a.R = op->i[4]; a.ldo = op->i[13];
  for (int c = 0; c < 3; ++c) { a.mean[c] = op->f[c]; a.stdv[c] = op->f[3 + c]; }
  OMNI_REQUIRE(a.n >= 1 && a.n <= kMaxTiles, "region_ocr cut: %d tiles (i1), 1..%d", a.n, kMaxTiles);
  OMNI_REQUIRE(a.H >= 1 && a.W >= 1, "region_ocr cut: a frame of %d x %d (i2 x i3)", a.H, a.W);
  OMNI_REQUIRE(a.R >= 1 && a.R <= kMaxR, "region_ocr cut: R = %d (i4), 1..%d", a.R, kMaxR);
  OMNI_REQUIRE(a.ldo >= 3 && a.ldo <= 64, "region_ocr cut: pixel pitch %d (i13), 3..64 elements", a.ldo);
  OMNI_REQUIRE(op->dtype == OMNI_F32 || op->dtype == OMNI_F16, "region_ocr cut: unsupported dtype %d", op->dtype);
  OMNI_REQUIRE(a.img && a.origins && a.y && a.lut, "region_ocr cut: p0 (frame), p1 (origins), p4 (tiles) or p7 (1/255 table) is NULL");
  OMNI_REQUIRE((unsigned long long)a.origins % 4 == 0 && (unsigned long long)a.lut % 4 == 0 &&
               (unsigned long long)a.y % (op->dtype == OMNI_F32 ? 4 : 2) == 0, "region_ocr cut: p1 / p4 / p7 not aligned to their elements");
  for (int c = 0; c < 3; ++c) OMNI_REQUIRE(a.stdv[c] != 0.0f, "region_ocr cut: std of channel %d (f%d) is 0", c, 3 + c);
  const dim3 grid((unsigned)(((long long)a.R * a.R + 255) / 256), a.n);
  if (op->dtype == OMNI_F32) hipLaunchKernelGGL(tile_cut_kernel<float>, grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL(tile_cut_kernel<half_t>, grid, dim3(256), 0, s, a);
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}

// ---------------------------------------------------------------------------------------------- mode 1
struct ParseArgs {
  const int* ids; const unsigned short* table; const float* logp; const int* cells;
  int* rec; float* sum; int* rows;
  int n, T, M, table_len, ld_ids, ld_logp, R, eos, grammar;
};

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

// one block of one wave per row
__global__ __launch_bounds__(64) void region_parse_kernel(ParseArgs a) {
  __shared__ unsigned short cls[kMaxT];        // class of ORIGINAL token j
  __shared__ unsigned short orig[kMaxT];       // original index of stripped token s
  __shared__ unsigned short ra[kMaxM], rb[kMaxM], rc[kMaxM];   // region k: original index of its first content token, first and last location token
  __shared__ int found, kept;
  const int lane = threadIdx.x, row = blockIdx.x;
  const int* ids = a.ids + (long long)row * a.ld_ids;
  int end = a.T;                               // the row is [1, end): in front of the first EOS behind the start token
  for (int j = 1 + lane; j < a.T; j += 64) {
    const int id = ids[j];
    int c = kHard;
    if (id >= 0 && id < a.table_len) c = min((int)a.table[id], kHard);
    cls[j] = (unsigned short)c;
    if (id == a.eos) end = min(end, j);
  }
  end = wave_min(end);
  __syncthreads();
  int hard = 0;
  for (int j = 1 + lane; j < end; j += 64) hard |= cls[j] == kHard;
  hard = wave_or(hard);
  if (lane == 0) {
    int s = 0, p = 0, run = 0, k = 0;          // stripped tokens so far, stripped index of the open region's start, location run, regions
    for (int j = 1; j < end; ++j) {
      const int c = cls[j];
      if (c == kStrip) continue;
      orig[s] = (unsigned short)j;
      run = c < 1000 ? run + 1 : 0;
      if (run >= 8 && s - 7 >= p + 1) {        // tokens s - 7 .. s are location tokens and at least one token of content is in front
        ra[k] = orig[p]; rb[k] = orig[s - 7]; rc[k] = (unsigned short)j;
        ++k;
        p = s + 1;
        run = 0;
      }
      ++s;
    }
    found = k;
    kept = 0;
  }
  __syncthreads();
  const int nreg = found;                      // <= (end - 1) / 9 <= M
  const int* cell = a.cells + (long long)row * 6;
  for (int k = lane; k < a.M; k += 64) {
    int* rec = a.rec + ((long long)row * a.M + k) * 16;
    if (k >= nreg) {
#pragma unroll
      for (int t = 0; t < 16; ++t) rec[t] = 0;
      a.sum[(long long)row * a.M + k] = 0.0f;
      continue;
    }
    const int first = ra[k], b = rb[k], last_loc = rc[k];
    int cnt = 0, last = first + 1, q = 0;
    long long lo[2] = {LLONG_MAX, LLONG_MAX}, hi[2] = {LLONG_MIN, LLONG_MIN};   // [0] x, [1] y over the four corners
    float sum = 0.0f;
    for (int j = first; j <= last_loc; ++j) {
      const int c = cls[j];
      if (c == kStrip) continue;
      ++cnt;
      if (a.logp) sum += a.logp[(long long)row * a.ld_logp + j - 1];
      if (j < b) { last = j + 1; continue; }
      const long long v = (long long)(((2 * c + 1) * a.R) / 2000) + cell[q & 1];   // exactly 8 tokens get here, all of them bins
      if (q & 1) { lo[1] = min(lo[1], v); hi[1] = max(hi[1], v); }
      else { lo[0] = min(lo[0], v); hi[0] = max(hi[0], v); }
      rec[3 + (q & 7)] = (int)v;
      ++q;
    }
    const long long cx = lo[0] + hi[0], cy = lo[1] + hi[1];                      // the box centre, doubled
    const bool own = cx >= cell[2] && (cell[3] == INT_MAX || cx < cell[3]) && cy >= cell[4] && (cell[5] == INT_MAX || cy < cell[5]);
    rec[0] = row; rec[1] = first; rec[2] = last;
    rec[11] = cnt; rec[12] = own; rec[13] = rec[14] = rec[15] = 0;
    a.sum[(long long)row * a.M + k] = sum;
    if (own) atomicAdd(&kept, 1);
  }
  __syncthreads();
  if (lane == 0) {
    int* r = a.rows + (long long)row * 4;
    r[0] = nreg; r[1] = kept; r[2] = hard | (end == a.T ? 2 : 0); r[3] = 0;
  }
}

// ---------------------------------------------------------------------------------------------- mode 3
// one block of one wave per row; ParseArgs as in mode 1 with M = (T - 1) / 4 box slots and sums of two floats per slot
__global__ __launch_bounds__(64) void region_boxes_kernel(ParseArgs a) {
  __shared__ unsigned short cls[kMaxT];        // class of ORIGINAL token j
  __shared__ unsigned short orig[kMaxT];       // original index of stripped token s
  __shared__ unsigned short ba[kMaxB], bb[kMaxB], bc[kMaxB], bp[kMaxB];   // box k: first and one-past-last column of its phrase, column of its
                                                                          // first location token, phrase ordinal | lead << 15
  __shared__ int found, kept, phrases;
  const int lane = threadIdx.x, row = blockIdx.x;
  const int* ids = a.ids + (long long)row * a.ld_ids;
  int end = a.T;                               // the row is [1, end): in front of the first EOS behind the start token
  for (int j = 1 + lane; j < a.T; j += 64) {
    const int id = ids[j];
    int c = kHard;
    if (id >= 0 && id < a.table_len) c = min((int)a.table[id], kHard);
    cls[j] = (unsigned short)c;
    if (id == a.eos) end = min(end, j);
  }
  end = wave_min(end);
  __syncthreads();
  int hard = 0;
  for (int j = 1 + lane; j < end; j += 64) hard |= cls[j] == kHard;
  hard = wave_or(hard);
  if (lane == 0) {
    int s = 0;
    for (int j = 1; j < end; ++j)
      if (cls[j] != kStrip) orig[s++] = (unsigned short)j;
    int i = 0, k = 0, ph = 0, carry = -1;      // stripped index, boxes, phrases, stripped index of a location token left to lead a phrase
    while (i < s) {
      const int t = i;
      while (i < s && cls[orig[i]] >= 1000) ++i;
      const int at = i;                        // text run [t, at), location run [at, i)
      while (i < s && cls[orig[i]] < 1000) ++i;
      const int r = i - at;
      int p0, p1, b0, nb, lead = 0;            // phrase [p0, p1) and nb boxes from b0, all stripped indices
      if (a.grammar == 1) {
        if (r < 4) continue;
        p0 = p1 = b0 = at; nb = r / 4;
      } else {
        const int start = carry >= 0 ? carry : (at > t ? t : -1);
        if (start >= 0 && r >= 4) { p0 = start; p1 = at; lead = carry >= 0; b0 = at; nb = r / 4; }
        else if (start < 0 && r >= 5) { p0 = at; p1 = at + 1; lead = 1; b0 = at + 1; nb = (r - 1) / 4; }
        else { carry = i - 1; continue; }      // (r = 0 only behind the row's last text run: nothing follows)
        carry = -1;
      }
      for (int q = 0; q < nb; ++q, ++k) {      // k < (s / 4) <= M: every box has four location tokens of its own
        const int first = orig[b0 + 4 * q];
        ba[k] = p1 > p0 ? orig[p0] : (unsigned short)first;
        bb[k] = p1 > p0 ? (unsigned short)(orig[p1 - 1] + 1) : (unsigned short)first;
        bc[k] = (unsigned short)first;
        bp[k] = (unsigned short)(ph | (lead << 15));
      }
      ++ph;
    }
    found = k;
    phrases = ph;
    kept = 0;
  }
  __syncthreads();
  const int nbox = found;
  const int* cell = a.cells + (long long)row * 6;
  for (int k = lane; k < a.M; k += 64) {
    int* rec = a.rec + ((long long)row * a.M + k) * 16;
    float* sum = a.sum + ((long long)row * a.M + k) * 2;
    if (k >= nbox) {
#pragma unroll
      for (int t = 0; t < 16; ++t) rec[t] = 0;
      sum[0] = sum[1] = 0.0f;
      continue;
    }
    const int c0 = ba[k], c1 = bb[k], cloc = bc[k];
    int cnt = 0, q = 0;
    float sp = 0.0f, sb = 0.0f;
    for (int j = c0; j < c1; ++j) {
      if (cls[j] == kStrip) continue;
      ++cnt;
      if (a.logp) sp += a.logp[(long long)row * a.ld_logp + j - 1];
    }
    long long v[4] = {0, 0, 0, 0};
    for (int j = cloc; j < end && q < 4; ++j) {                                  // the walk saw four location tokens from here
      const int c = cls[j];
      if (c == kStrip) continue;
      if (a.logp) sb += a.logp[(long long)row * a.ld_logp + j - 1];
      v[q] = (long long)(((2 * c + 1) * a.R) / 2000) + cell[q & 1];
      ++q;
    }
    const long long cx = v[0] + v[2], cy = v[1] + v[3];                           // the box centre, doubled
    const bool own = cx >= cell[2] && (cell[3] == INT_MAX || cx < cell[3]) && cy >= cell[4] && (cell[5] == INT_MAX || cy < cell[5]);
    rec[0] = row; rec[1] = c0; rec[2] = c1;
    rec[3] = (int)v[0]; rec[4] = (int)v[1]; rec[5] = (int)v[2]; rec[6] = (int)v[3];
    rec[7] = cloc; rec[8] = cnt; rec[9] = own; rec[10] = bp[k] & 0x7fff; rec[11] = bp[k] >> 15;
    rec[12] = rec[13] = rec[14] = rec[15] = 0;
    sum[0] = sp; sum[1] = sb;
    if (own) atomicAdd(&kept, 1);
  }
  __syncthreads();
  if (lane == 0) {
    int* r = a.rows + (long long)row * 4;
    r[0] = nbox; r[1] = kept; r[2] = hard | (end == a.T ? 2 : 0); r[3] = phrases;
  }
}

// ---------------------------------------------------------------------------------------------- mode 5
struct PolyArgs {
  const int* ids; const unsigned short* table; const float* logp; const int* cells;
  int* verts; int* rec; float* sum; int* rows;
  int n, T, P, V, table_len, ld_ids, ld_logp, R, eos;
};

__device__ __forceinline__ bool is_structure(int c) { return c < 1000 || c >= kSep; }   // classes are clamped to 0..kPolyEnd

// one block of one wave per row
__global__ __launch_bounds__(64) void region_polys_kernel(PolyArgs a) {
  __shared__ unsigned short cls[kMaxT];        // class of ORIGINAL token j
  __shared__ unsigned short orig[kMaxT];       // original index of stripped token s
  __shared__ unsigned short pc0[kMaxP], pc1[kMaxP], pnl[kMaxP], pin[kMaxP], por[kMaxP], pru[kMaxP], pv0[kMaxP], pkp[kMaxP];
  // polygon k: columns of its first location token and one past its last, location tokens, instance, ordinal in it, run, first vertex
  // slot; pkp: the instance's kept flag, at its first polygon
  __shared__ int bx0[kMaxP], by0[kMaxP], bx1[kMaxP], by1[kMaxP];     // polygon k's own box, then (at an instance's first polygon) the instance's
  __shared__ int found, insts, kept, nverts;
  const int lane = threadIdx.x, row = blockIdx.x;
  const int* ids = a.ids + (long long)row * a.ld_ids;
  int end = a.T;                               // the row is [1, end): in front of the first EOS behind the start token
  for (int j = 1 + lane; j < a.T; j += 64) {
    const int id = ids[j];
    int c = kHard;
    if (id >= 0 && id < a.table_len) { c = a.table[id]; if (c > kPolyEnd) c = kHard; }
    cls[j] = (unsigned short)c;
    if (id == a.eos) end = min(end, j);
  }
  end = wave_min(end);
  __syncthreads();
  int hard = 0;
  for (int j = 1 + lane; j < end; j += 64) hard |= cls[j] == kHard;
  hard = wave_or(hard);
  if (lane == 0) {
    int s = 0;
    for (int j = 1; j < end; ++j)
      if (cls[j] != kStrip) orig[s++] = (unsigned short)j;
    int i = 0, k = 0, inst = 0, run = 0, nv = 0;   // stripped index, polygons, instances, runs of four or more, vertices
    while (i < s) {
      if (!is_structure(cls[orig[i]])) { ++i; continue; }
      const int ra = i;
      bool open = false, close = false;
      for (; i < s && is_structure(cls[orig[i]]); ++i) { open |= cls[orig[i]] == kPoly; close |= cls[orig[i]] == kPolyEnd; }
      const int rb = i;                        // the run [ra, rb)
      if (rb - ra < 4) continue;
      const int this_run = run++;
      bool ahead = false;                      // a location token or <poly> behind ONE leading location token
      for (int q = ra + (cls[orig[ra]] < 1000); q < rb && !ahead; ++q) ahead = cls[orig[q]] < 1000 || cls[orig[q]] == kPoly;
      if (!ahead) continue;
      const bool pairs = open && close;
      for (int pos = ra;;) {
        int cs = ra, ce = rb;                  // the instance's content [cs, ce)
        if (pairs) {
          while (pos < rb && cls[orig[pos]] != kPoly) ++pos;
          if (pos >= rb) break;
          cs = ce = pos + 1;
          while (ce < rb && cls[orig[ce]] != kPolyEnd) ++ce;
          if (ce >= rb) break;
          pos = ce + 1;
        }
        int ord = 0;
        for (int j = cs; j < ce;) {
          if (cls[orig[j]] >= 1000) { ++j; continue; }
          int e = j;
          while (e < ce && cls[orig[e]] < 1000) ++e;
          if ((e == ce || cls[orig[e]] == kSep) && k < a.P) {     // k < T / 2 always: a polygon has a location token and, but the last, a token behind it
            pc0[k] = orig[j]; pc1[k] = (unsigned short)(orig[e - 1] + 1); pnl[k] = (unsigned short)(e - j);
            pin[k] = (unsigned short)inst; por[k] = (unsigned short)ord; pru[k] = (unsigned short)this_run; pv0[k] = (unsigned short)nv;
            nv += (e - j) / 2;
            ++k; ++ord;
          }
          j = e < ce ? e + 1 : e;
        }
        if (ord) ++inst;
        if (!pairs) break;
      }
    }
    found = k; insts = inst; nverts = nv; kept = 0;
  }
  __syncthreads();
  const int npoly = found, total = nverts;     // total <= (end - 1) / 2 <= V: a vertex is two location tokens of its own
  const int* cell = a.cells + (long long)row * 6;
  int* verts = a.verts + (long long)row * a.V * 2;
  for (int v = total + lane; v < a.V; v += 64) verts[2 * v] = verts[2 * v + 1] = 0;
  for (int k = lane; k < a.P; k += 64) {
    float* sum = a.sum + (long long)row * a.P + k;
    if (k >= npoly) {
      int* rec = a.rec + ((long long)row * a.P + k) * 16;
#pragma unroll
      for (int t = 0; t < 16; ++t) rec[t] = 0;
      *sum = 0.0f;
      continue;
    }
    const int want = 2 * (pnl[k] / 2), v0 = pv0[k];               // an odd number of bins drops the last one
    int lo[2] = {INT_MAX, INT_MAX}, hi[2] = {INT_MIN, INT_MIN}, q = 0;
    float sp = 0.0f;
    for (int j = pc0[k]; j < end && q < want; ++j) {              // the walk saw pnl[k] location tokens from here
      const int c = cls[j];
      if (c == kStrip) continue;
      if (a.logp) sp += a.logp[(long long)row * a.ld_logp + j - 1];
      const int v = ((2 * c + 1) * a.R) / 2000 + cell[q & 1];
      lo[q & 1] = min(lo[q & 1], v); hi[q & 1] = max(hi[q & 1], v);
      if (v0 + q / 2 < a.V) verts[2 * (v0 + q / 2) + (q & 1)] = v;
      ++q;
    }
    bx0[k] = lo[0]; by0[k] = lo[1]; bx1[k] = hi[0]; by1[k] = hi[1];
    *sum = sp;
  }
  __syncthreads();
  for (int k = lane; k < npoly; k += 64) {
    if (por[k]) continue;                      // the lane of an instance's first polygon folds the instance's box
    int x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
    for (int m = k; m < npoly && pin[m] == pin[k]; ++m) {
      x0 = min(x0, bx0[m]); y0 = min(y0, by0[m]); x1 = max(x1, bx1[m]); y1 = max(y1, by1[m]);
    }
    bool own = false;
    if (x0 == INT_MAX) x0 = y0 = x1 = y1 = 0;  // no vertex at all
    else {
      const long long cx = (long long)x0 + x1, cy = (long long)y0 + y1;
      own = cx >= cell[2] && (cell[3] == INT_MAX || cx < cell[3]) && cy >= cell[4] && (cell[5] == INT_MAX || cy < cell[5]);
    }
    bx0[k] = x0; by0[k] = y0; bx1[k] = x1; by1[k] = y1; pkp[k] = own;
    if (own) atomicAdd(&kept, 1);
  }
  __syncthreads();
  for (int k = lane; k < npoly; k += 64) {
    int* rec = a.rec + ((long long)row * a.P + k) * 16;
    const int k0 = k - por[k];
    rec[0] = row; rec[1] = pin[k]; rec[2] = por[k]; rec[3] = pv0[k]; rec[4] = pnl[k] / 2; rec[5] = pc0[k]; rec[6] = pc1[k];
    rec[7] = pnl[k]; rec[8] = pkp[k0]; rec[9] = pru[k]; rec[10] = bx0[k0]; rec[11] = by0[k0]; rec[12] = bx1[k0]; rec[13] = by1[k0];
    rec[14] = rec[15] = 0;
  }
  if (lane == 0) {
    int* r = a.rows + (long long)row * 4;
    r[0] = npoly; r[1] = insts; r[2] = hard | (end == a.T ? 2 : 0); r[3] = kept;
  }
}

// ---------------------------------------------------------------------------------------------- mode 6
struct MaskArgs {
  const int* rec; const int* rows; const int* verts; const int* cells; unsigned* mask; int* cnt;
  int n, P, V, I, H, W, R;
};

// block (x, y, z) = (four pixel rows, instance slot, row); one wave per pixel row
__global__ __launch_bounds__(256) void poly_mask_kernel(MaskArgs a) {
  __shared__ int vx[kMaxV], vy[kMaxV];         // the instance's vertices, tile-local
  __shared__ unsigned short ps[kMaxP], pn[kMaxP];   // polygon p of the instance: its first vertex in vx / vy, its vertices (0 = skip)
  __shared__ int first, npoly, vend;
  const int tid = threadIdx.x, lane = tid & 63, y = blockIdx.x * 4 + (tid >> 6), s = blockIdx.y;
  const int WR = (a.R + 31) / 32;
  for (int row = blockIdx.z; row < a.n; row += gridDim.z) {
    __syncthreads();                           // the row before is done with the LDS
    if (tid == 0) { first = -1; npoly = 0; vend = 0; }
    __syncthreads();
    const int* rec = a.rec + (long long)row * a.P * 16;
    const int found = min(max(a.rows[(long long)row * 4], 0), a.P);
    for (int k = tid; k < found; k += 256)
      if (rec[k * 16 + 1] == s && rec[k * 16 + 2] == 0) first = k;            // the instance's first polygon: one record at most
    __syncthreads();
    const int k0 = first;
    const int ox = a.cells[(long long)row * 6], oy = a.cells[(long long)row * 6 + 1];
    bool live = k0 >= 0 && rec[k0 * 16 + 8] != 0;                             // block-uniform
    int ylo = 0, yhi = 0, vbeg = 0;
    if (live) {
      vbeg = rec[k0 * 16 + 3];
      ylo = rec[k0 * 16 + 11] - oy; yhi = rec[k0 * 16 + 13] - oy;            // edges span the pixel rows ylo <= y < yhi only
      live = vbeg >= 0 && vbeg < a.V;
    }
    if (live) {
      const int room = min(a.V - vbeg, kMaxV);                                // vertices that may be staged
      for (int k = k0 + tid; k < found; k += 256) {                           // found <= P <= kMaxP
        if (rec[k * 16 + 1] != s) continue;                                    // (the instance's records are consecutive)
        const int rel = rec[k * 16 + 3] - vbeg, nv = rec[k * 16 + 4];
        const bool ok = rel >= 0 && nv >= 0 && rel <= room && nv <= room - rel;
        ps[k - k0] = (unsigned short)(ok ? rel : 0); pn[k - k0] = (unsigned short)(ok && nv >= 3 ? nv : 0);
        atomicAdd(&npoly, 1);
        if (ok && (k + 1 == found || rec[(k + 1) * 16 + 1] != s)) vend = rel + nv;   // the last polygon ends the instance's vertices
      }
      __syncthreads();
      const int* verts = a.verts + ((long long)row * a.V + vbeg) * 2;
      for (int v = tid; v < vend; v += 256) { vx[v] = verts[2 * v] - ox; vy[v] = verts[2 * v + 1] - oy; }
      for (int p = tid; p < npoly; p += 256)
        if (ps[p] + pn[p] > vend) pn[p] = 0;                                   // (records that are not mode 5's: nothing unstaged is read)
      __syncthreads();
    }
    if (y >= a.R) continue;                    // wave-uniform; the barriers above are behind it
    unsigned* mrow = a.mask + (((long long)row * a.I + s) * a.R + y) * WR;
    const bool rowlive = live && y >= ylo && y < yhi && (long long)oy + y >= 0 && (long long)oy + y < a.H;
    if (!rowlive) {
      for (int w = lane; w < WR; w += 64) mrow[w] = 0u;
      if (lane == 0) a.cnt[((long long)row * a.I + s) * a.R + y] = 0;
      continue;
    }
    const int np = npoly;
    int set = 0;                               // lanes 0 and 32: set bits of the words they wrote
    for (int w0 = 0; w0 < WR; w0 += 2) {
      const int x = w0 * 32 + lane;
      int in = 0;
      if (x < a.R && (long long)ox + x >= 0 && (long long)ox + x < a.W) {
        const long long px = 2LL * x + 1, py = 2LL * y + 1;
        for (int p = 0; p < np; ++p) {
          const int nv = pn[p], b = ps[p];
          if (nv < 3) continue;
          long long ax = 2LL * vx[b + nv - 1], ay = 2LL * vy[b + nv - 1];
          int par = 0;
          for (int e = 0; e < nv; ++e) {
            const long long ex = 2LL * vx[b + e], ey = 2LL * vy[b + e];
            if ((ay > py) != (ey > py)) {
              const long long l = (px - ax) * (ey - ay), r = (py - ay) * (ex - ax);
              par ^= ey > ay ? l < r : l > r;
            }
            ax = ex; ay = ey;
          }
          in |= par;
        }
      }
      unsigned word = (unsigned)in << (lane & 31);
#pragma unroll
      for (int o = 16; o > 0; o >>= 1) word |= __shfl_xor(word, o);           // OR over the half-wave
      const int w = w0 + (lane >> 5);
      if ((lane & 31) == 0 && w < WR) { mrow[w] = word; set += __popcll((unsigned long long)word); }
    }
    const int upper = __shfl(set, 32);
    if (lane == 0) a.cnt[((long long)row * a.I + s) * a.R + y] = set + upper;
  }
}

int parse_cfg(const omni_op_t* op, ParseArgs& a) {
  const bool boxes = op->i[0] == 3;
  a.n = op->i[1]; a.T = op->i[2]; a.M = op->i[3]; a.table_len = op->i[4];
  a.ld_ids = op->i[5] ? op->i[5] : a.T; a.ld_logp = op->i[6] ? op->i[6] : a.T - 1; a.R = op->i[7]; a.eos = op->i[8];
  a.grammar = boxes ? op->i[9] : 0;
  OMNI_REQUIRE(a.n >= 1 && a.n <= kMaxTiles, "region_ocr parse: %d rows (i1), 1..%d", a.n, kMaxTiles);
  OMNI_REQUIRE(a.T >= 2 && a.T <= kMaxT, "region_ocr parse: rows of T = %d tokens (i2), 2..%d", a.T, kMaxT);
  if (boxes) {
    OMNI_REQUIRE(a.M == (a.T - 1) / 4, "region_ocr boxes: %d box slots per row (i3), (T - 1) / 4 = %d", a.M, (a.T - 1) / 4);
    OMNI_REQUIRE(a.grammar == 0 || a.grammar == 1, "region_ocr boxes: grammar %d (i9), 0 = phrases with boxes, 1 = boxes only", a.grammar);
  } else {
    OMNI_REQUIRE(a.M == (a.T - 1) / 9, "region_ocr parse: %d region slots per row (i3), (T - 1) / 9 = %d", a.M, (a.T - 1) / 9);
  }
  OMNI_REQUIRE(a.table_len >= 1, "region_ocr parse: a class table of %d entries (i4)", a.table_len);
  OMNI_REQUIRE(a.ld_ids >= a.T && a.ld_logp >= a.T - 1, "region_ocr parse: row strides %d (i5) / %d (i6) below T = %d / T - 1", a.ld_ids, a.ld_logp, a.T);
  OMNI_REQUIRE(a.R >= 1 && a.R <= kMaxR, "region_ocr parse: R = %d (i7), 1..%d", a.R, kMaxR);
  return OMNI_OK;
}

int launch_parse(const omni_op_t* op, hipStream_t s) {
  ParseArgs a{};
  if (int rc = parse_cfg(op, a)) return rc;
  a.ids = (const int*)op->p[0]; a.table = (const unsigned short*)op->p[1]; a.logp = (const float*)op->p[2];
  a.rec = (int*)op->p[4]; a.sum = (float*)op->p[5]; a.rows = (int*)op->p[6]; a.cells = (const int*)op->p[7];
  OMNI_REQUIRE(a.ids && a.table && a.rec && a.sum && a.rows && a.cells,
               "region_ocr parse: p0 (ids), p1 (class table), p4 (records), p5 (sums), p6 (row counters) or p7 (cells) is NULL");
  OMNI_REQUIRE((unsigned long long)a.ids % 4 == 0 && (unsigned long long)a.table % 2 == 0 && (unsigned long long)a.logp % 4 == 0 &&
               (unsigned long long)a.rec % 4 == 0 && (unsigned long long)a.sum % 4 == 0 && (unsigned long long)a.rows % 4 == 0 &&
               (unsigned long long)a.cells % 4 == 0, "region_ocr parse: a pointer is not aligned to its elements");
  if (op->i[0] == 3) hipLaunchKernelGGL(region_boxes_kernel, dim3(a.n), dim3(64), 0, s, a);
  else hipLaunchKernelGGL(region_parse_kernel, dim3(a.n), dim3(64), 0, s, a);
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}

int polys_cfg(const omni_op_t* op, PolyArgs& a) {
  a.n = op->i[1]; a.T = op->i[2]; a.P = op->i[3]; a.table_len = op->i[4];
  a.ld_ids = op->i[5] ? op->i[5] : a.T; a.ld_logp = op->i[6] ? op->i[6] : a.T - 1; a.R = op->i[7]; a.eos = op->i[8]; a.V = op->i[9];
  OMNI_REQUIRE(a.n >= 1 && a.n <= kMaxTiles, "region_ocr polys: %d rows (i1), 1..%d", a.n, kMaxTiles);
  OMNI_REQUIRE(a.T >= 3 && a.T <= kMaxT, "region_ocr polys: rows of T = %d tokens (i2), 3..%d", a.T, kMaxT);
  OMNI_REQUIRE(a.P == a.T / 2, "region_ocr polys: %d polygon slots per row (i3), T / 2 = %d", a.P, a.T / 2);
  OMNI_REQUIRE(a.V == (a.T - 1) / 2, "region_ocr polys: %d vertex slots per row (i9), (T - 1) / 2 = %d", a.V, (a.T - 1) / 2);
  OMNI_REQUIRE(a.table_len >= 1, "region_ocr polys: a class table of %d entries (i4)", a.table_len);
  OMNI_REQUIRE(a.ld_ids >= a.T && a.ld_logp >= a.T - 1, "region_ocr polys: row strides %d (i5) / %d (i6) below T = %d / T - 1", a.ld_ids, a.ld_logp, a.T);
  OMNI_REQUIRE(a.R >= 1 && a.R <= kMaxR, "region_ocr polys: R = %d (i7), 1..%d", a.R, kMaxR);
  return OMNI_OK;
}

int launch_polys(const omni_op_t* op, hipStream_t s) {
  PolyArgs a{};
  if (int rc = polys_cfg(op, a)) return rc;
  a.ids = (const int*)op->p[0]; a.table = (const unsigned short*)op->p[1]; a.logp = (const float*)op->p[2]; a.verts = (int*)op->p[3];
  a.rec = (int*)op->p[4]; a.sum = (float*)op->p[5]; a.rows = (int*)op->p[6]; a.cells = (const int*)op->p[7];
  OMNI_REQUIRE(a.ids && a.table && a.verts && a.rec && a.sum && a.rows && a.cells,
               "region_ocr polys: p0 (ids), p1 (class table), p3 (vertices), p4 (records), p5 (sums), p6 (row counters) or p7 (cells) is NULL");
  OMNI_REQUIRE((unsigned long long)a.ids % 4 == 0 && (unsigned long long)a.table % 2 == 0 && (unsigned long long)a.logp % 4 == 0 &&
               (unsigned long long)a.verts % 4 == 0 && (unsigned long long)a.rec % 4 == 0 && (unsigned long long)a.sum % 4 == 0 &&
               (unsigned long long)a.rows % 4 == 0 && (unsigned long long)a.cells % 4 == 0, "region_ocr polys: a pointer is not aligned to its elements");
  hipLaunchKernelGGL(region_polys_kernel, dim3(a.n), dim3(64), 0, s, a);
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}

int masks_cfg(const omni_op_t* op, MaskArgs& a) {
  a.n = op->i[1]; a.P = op->i[2] / 2; a.V = (op->i[2] - 1) / 2; a.I = op->i[3]; a.H = op->i[4]; a.W = op->i[5]; a.R = op->i[7];
  OMNI_REQUIRE(a.n >= 1 && a.n <= kMaxTiles, "region_ocr masks: %d rows (i1), 1..%d", a.n, kMaxTiles);
  OMNI_REQUIRE(op->i[2] >= 3 && op->i[2] <= kMaxT, "region_ocr masks: rows of T = %d tokens (i2), 3..%d", op->i[2], kMaxT);
  OMNI_REQUIRE(a.I >= 1 && a.I <= kMaxI, "region_ocr masks: %d instance slots per row (i3), 1..%d", a.I, kMaxI);
  OMNI_REQUIRE(a.H >= 1 && a.W >= 1, "region_ocr masks: a frame of %d x %d (i4 x i5)", a.H, a.W);
  OMNI_REQUIRE(a.R >= 1 && a.R <= kMaxR, "region_ocr masks: R = %d (i7), 1..%d", a.R, kMaxR);
  return OMNI_OK;
}

int launch_masks(const omni_op_t* op, hipStream_t s) {
  MaskArgs a{};
  if (int rc = masks_cfg(op, a)) return rc;
  a.rec = (const int*)op->p[0]; a.rows = (const int*)op->p[1]; a.verts = (const int*)op->p[2]; a.mask = (unsigned*)op->p[4];
  a.cnt = (int*)op->p[5]; a.cells = (const int*)op->p[7];
  OMNI_REQUIRE(a.rec && a.rows && a.verts && a.mask && a.cnt && a.cells,
               "region_ocr masks: p0 (records), p1 (row counters), p2 (vertices), p4 (masks), p5 (counts) or p7 (cells) is NULL");
  OMNI_REQUIRE((unsigned long long)a.rec % 4 == 0 && (unsigned long long)a.rows % 4 == 0 && (unsigned long long)a.verts % 4 == 0 &&
               (unsigned long long)a.mask % 4 == 0 && (unsigned long long)a.cnt % 4 == 0 && (unsigned long long)a.cells % 4 == 0,
               "region_ocr masks: a pointer is not aligned to its elements");
  hipLaunchKernelGGL(poly_mask_kernel, dim3((a.R + 3) / 4, a.I, min(a.n, 65535)), dim3(256), 0, s, a);
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}

}  // namespace

// the bytes modes 1, 3, 5 and 6 touch behind p0 .. p7; false for an op whose slots the launcher refuses (capi.hip::op_extents)
bool omni_region_ocr_extents(const omni_op_t* op, long long ext[8]) {
  if (op->i[0] == 5) {
    PolyArgs a{};
    if (polys_cfg(op, a) != OMNI_OK) return false;
    ext[0] = ((long long)(a.n - 1) * a.ld_ids + a.T) * 4;
    ext[1] = (long long)a.table_len * 2;
    ext[2] = ((long long)(a.n - 1) * a.ld_logp + a.T - 1) * 4;
    ext[3] = (long long)a.n * a.V * 8;
    ext[4] = (long long)a.n * a.P * 64; ext[5] = (long long)a.n * a.P * 4; ext[6] = (long long)a.n * 16; ext[7] = (long long)a.n * 24;
    return true;
  }
  if (op->i[0] == 6) {
    MaskArgs a{};
    if (masks_cfg(op, a) != OMNI_OK) return false;
    ext[0] = (long long)a.n * a.P * 64; ext[1] = (long long)a.n * 16; ext[2] = (long long)a.n * a.V * 8;
    ext[4] = (long long)a.n * a.I * a.R * ((a.R + 31) / 32) * 4; ext[5] = (long long)a.n * a.I * a.R * 4; ext[7] = (long long)a.n * 24;
    return true;
  }
  ParseArgs a{};
  if (parse_cfg(op, a) != OMNI_OK) return false;
  ext[0] = ((long long)(a.n - 1) * a.ld_ids + a.T) * 4;
  ext[1] = (long long)a.table_len * 2;
  ext[2] = ((long long)(a.n - 1) * a.ld_logp + a.T - 1) * 4;
  ext[4] = (long long)a.n * a.M * 64; ext[5] = (long long)a.n * a.M * (op->i[0] == 3 ? 8 : 4); ext[6] = (long long)a.n * 16; ext[7] = (long long)a.n * 24;
  return true;
}

int omni_launch_region_ocr(const omni_op_t* op, hipStream_t s) {
  const int mode = op->i[0];
  if (mode == 0) return launch_cut(op, s);
  if (mode == 5) return launch_polys(op, s);
  if (mode == 6) return launch_masks(op, s);
  OMNI_REQUIRE(mode == 1 || mode == 3, "region_ocr: mode %d (i0), 0 = tile cut, 1 = region parse, 3 = box parse, 5 = polygon parse, 6 = mask raster", mode);
  return launch_parse(op, s);
}
