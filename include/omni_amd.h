/*
 * omni_amd.h — C ABI of libomni_amd.so, the MI355X (gfx950) screen-parsing hot path.
 *
 * The reference (microsoft/OmniParser) has no FFI: its hot path is Python calling
 * third-party kernels (TorchScript YOLOv9-E, torchvision::nms, transformers
 * Florence-2).  This header is the boundary a maintainer binds with ctypes from
 * the reference's own adapter classes (INTEGRATION.md shows the stubs).  Each
 * entry point cites the reference call it replaces (ref: = /root/reference,
 * hf: = site-packages/transformers).
 *
 * Conventions
 *   - plain pointers + sizes; every pointer named d_* is DEVICE memory owned by
 *     the caller (torch tensors in the Python host), h_* is host memory.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every
 *     call is asynchronous on that stream unless documented otherwise.
 *   - return 0 on success, negative OMNI_E_* on failure; omni_last_error()
 *     returns a thread-local message.
 *   - activations are NHWC (tokens x channels for the captioner), dtype
 *     OMNI_F32 (f32 storage, accumulation and statistics; GEMMs multiply on the f16
 *     matrix cores with both operands split into two f16 halves and THREE products
 *     per MAC — measured < 2e-6 relative to f64, the parity mode; short-K layers use
 *     the exact f32 MFMA) or OMNI_F16 (f16 storage and MFMA, f32 accumulate).
 */
#ifndef OMNI_AMD_H
#define OMNI_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 5): omni_stream_create / omni_stream_destroy / omni_plan_run_split and omni_debug_host_op are gone; OMNI_OP_ATTN_ROWS i17,
 * OMNI_OP_CHAN_ATTN i7 and OMNI_OP_CONV p6 are ignored (i22 / i23 = tile / split-K override); OMNI_OP_NMS sorts candidates inside the op.  A host compiled against
 * version 1 must be rebuilt: omni_abi_version() is what it checks at load time (omniparser_amd/_lib.py does). */
/* 3 (round 6): + omni_overflow_count; plan bundles carry the ABI version they were written under (omni_model_load rejects others). */
#define OMNI_ABI_VERSION 3

enum { OMNI_F32 = 0, OMNI_F16 = 1 };
enum { OMNI_ACT_NONE = 0, OMNI_ACT_SILU = 1, OMNI_ACT_GELU = 2 };
enum {
  OMNI_OK = 0,
  OMNI_E_ARG = -1,     /* bad argument / unsupported shape */
  OMNI_E_HIP = -2,     /* HIP runtime error */
  OMNI_E_NODEV = -3    /* no gfx950 device */
};

const char* omni_last_error(void);
int omni_abi_version(void);
/* number of visible HIP devices, <0 on error. */
int omni_device_count(void);
/* Range guard of the split-f16 formats (ABI 3).  OMNI_F32 plans keep the hi half of every GEMM operand in f16, so an activation
 * with |x| > 65504 cannot be represented (format B clamps it, format A loses it); the fp32 reference has no such limit
 * (ref:util/utils.py:66 loads the captioner in float32 on the CPU).  Every kernel that produces such an operand counts the
 * threads that saw a value beyond the range; *count = that number since the last reset (0 on every tensor of a healthy model).
 * Synchronous (a device-to-host copy of a few words): call it where the host already waits for results.  reset != 0 zeroes the
 * counters. */
int omni_overflow_count(int reset, unsigned long long* count);

/* ------------------------------------------------------------------------ *
 * Generic op descriptor: the plan executor and the single-op entry point
 * share it.  Slot meaning per kind is documented at each OMNI_OP_* below.
 * ------------------------------------------------------------------------ */
typedef struct omni_op {
  int32_t kind;      /* OMNI_OP_* */
  int32_t dtype;     /* OMNI_F32 / OMNI_F16: activation + weight element type */
  void*   p[8];      /* device pointers */
  int32_t i[32];     /* integer parameters */
  float   f[8];      /* float parameters */
} omni_op_t;

enum {
  /* Implicit-GEMM convolution / linear layer on MFMA, fused bias + act + residual.
   * Replaces the Conv2d(+BN)+SiLU stack inside the TorchScript detector
   * (ref:util/yolov9.py:121) and nn.Linear/Conv2d in the captioner
   * (hf:models/florence2/modeling_florence2.py, hf:models/bart/modeling_bart.py).
   *  p0 x [B,H,W,ldi]   p1 w [Cout][KH*KW*Cin] (k = (r*KW+s)*Cin + c)   p2 bias f32[Cout] or NULL
   *  p3 residual [M,ldr] or NULL   p4 y [B,Ho,Wo,ldo]
   *  i0 B i1 H i2 W i3 Cin i4 ldi i5 in_coff i6 KH i7 KW i8 stride i9 pad i10 Ho i11 Wo
   *  i12 Cout i13 ldo i14 out_coff i15 act i16 ldr i17 res_coff
   *  p5 optional split-K workspace (f32), i19 its size in KiB   f0 output scale (0 => 1)
   *  i20 = 1: split-f16 mode (f32 activations; w = [Cout][K/16][16 hi | 16 lo] f16 halves with w = hi + lo*2^-11;
   *           three f16 MFMAs per block give f32-class accuracy at the f16 matrix rate; needs Cin % 32 == 0)
   *  i20 = 2: pre-split LDS-DMA GEMM (csrc/gemm_dma.hip; pointwise layers only, K % 32 == 0, Cout % 128 == 0):
   *           BOTH operands are "format B" f16 pairs — a 16-channel group is 64 bytes, 16 hi halves then 16 lo halves,
   *           value = hi + lo (4 bytes per element, same strides as f32) — x written that way by its producer
   *           (OMNI_OP_LAYERNORM i6, this op's i21, OMNI_OP_SPLIT_CONVERT), w = split(W * 2^k) with f1 = 2^-k;
   *           i21 = 1: write y in format B as well (bias + activation applied first; no residual)
   *           i26 = n > 0 (additive; 0 = one weight matrix): PER-IMAGE WEIGHTS.  Rows [b n, (b + 1) n) of x are image b (M % n == 0) and
   *           multiply weight matrix b: p1 + b * i27 bytes (i27 % 16 == 0, i27 >= Cout * K * 4, or 0 = every image reads p1), each a
   *           format-B matrix of its own with its own power of two: p6 = f32[M / n] of 2^-k, read in place of f1 (NULL = f1 for all).
   *           n must be a multiple of the row tile the launcher takes (256, or 128 for short token matrices / OMNI_GEMM_TILE=128x128),
   *           else OMNI_E_ARG: the image of a tile is then uniform (n % 256 != 0 takes the 128-row tile).  Written by OMNI_OP_CHAN_ATTN's
   *           fold mode (i8 = 1).  i27 = 0 with p6 set = one shared weight and a 2^-k per image: the fold GEMM W''_b = W'_b . Wv of a channel
   *           block with Wv folded in (x = the packed per-image matrices, B * C rows of C, n = C; w = Wv^T packed on the host; p6[b] = the
   *           product of the image's 2^-k and the weight's 2^-kv, written by OMNI_OP_CHAN_ATTN i11 = 1; y = f32 [B][C][C])
   *  i29 = 1 (i20 = 2 with i26 > 0 only, additive; 0 = p2 is one bias vector): PER-IMAGE BIAS.  p2 = f32[M / i26][Cout], 16-byte aligned;
   *           the rows of image b add p2 + b * Cout.  Without per-image mode, with the scores epilogue, with p2 NULL or misaligned:
   *           OMNI_E_ARG.  The same vector in every row of the table gives the bits of the shared-bias launch
   *  i28 = 1 (i20 = 2 only, additive; 0 = the epilogues above): SCORES EPILOGUE for the q|k launch of a folded channel block.  The weight
   *           rows (and the bias) are ordered [q_0 | k_0 | q_1 | k_1 | ...], 32 rows per part, so that columns [64 g, 64 g + 64) of the
   *           product are q and k of channel group g.  Nothing is written to p4 (it may be NULL and is not touched); every 256-row tile
   *           is reduced to S[i][j] = sum_n q_g[n][i] k_g[n][j] over its rows (exact f32 products on the matrix pipe, in the summation
   *           order of OMNI_OP_CHAN_ATTN at i5 = 256, bit for bit) and stored to p7 = f32[M / 256 * Cout / 64 * 1024] at
   *           ((b * G + g) * chunks + chunk) * 1024 + i * 32 + j with G = Cout / 64, i26 = rows per image (> 0, % 256 == 0, M % i26 == 0;
   *           i27 = 0 and p6 = NULL keep the one weight matrix), b = row / i26, chunks = i26 / 256: the workspace layout of
   *           OMNI_OP_CHAN_ATTN, which then runs with i9 = 1.  Forces the 256x256 tile; needs Cout % 256 == 0, no activation, no residual,
   *           i21 = 0 and a non-NULL p7, else OMNI_E_ARG
   *  i22 (i20 = 0 or 1; 0 = the launcher's heuristic): output tile (1 = 64x64, 2 = 128x64, 3 = 128x128).  With i20 = 0 the K-slice
   *           width and the split-K count still follow from the tile as they do unforced (128-row tiles walk 64-byte slices)
   *  i23 (i20 = 1 only, ignored otherwise; 0 = the heuristic): split-K count (1 = no split, no reduce launch).  i22 / i23 are the
   *           per-shape choices of a tuning table; the sums differ only in the order of the K partials
   *  i24 = n > 0 (i20 = 1 only; round 6): p6 = int32[n] ARRIVAL COUNTERS, all zero before the first launch that uses them.  A split-K
   *           launch with at most n output tiles then combines its partials INSIDE the conv launch (each split publishes its tile
   *           write-through and draws a ticket; the last arriver sums in split order, applies bias / act / residual and zeroes the
   *           counter) instead of a second reduce launch: same sums in the same order, one launch less per conv.  Launches that share
   *           counters (or the workspace p5) must not run concurrently: one plan = one stream.  i24 = 0: the reduce launch
   *  i25 = 1 (i20 = 1 only; round 6): ROW-PATCH mode for a k x k convolution over ldi = 4 stored channels (k <= 8; the captioner's
   *           first patch embedding): pass it as a k x 1 convolution over 8 consecutive pixels — i6 KH = k, i7 KW = 1, i3 Cin = 32,
   *           i4 ldi = 4, i5 = 0, i8 / i9 stride / pad of BOTH axes, w = [Cout][k][8 pixels][4] with zero weights for pixel >= k (split
   *           like any i20 = 1 weight).  Pixels outside the image read as zero one by one; nothing is read beyond a row */
  OMNI_OP_CONV = 1,
  /* avg_pool2d(k=2,s=1,p=0) (ADown, ref blob T1).  p0 x, p4 y.
   *  i0 B i1 H i2 W i3 C i4 ldi i5 in_coff i13 ldo i14 out_coff (Ho=H-1, Wo=W-1) */
  OMNI_OP_AVGPOOL2 = 2,
  /* max_pool2d(k,s,p) with -inf padding (ADown k3s2p1, SPP k5s1p2).
   *  p0 x p4 y; i0 B i1 H i2 W i3 C i4 ldi i5 in_coff i6 k i8 stride i9 pad i10 Ho i11 Wo i13 ldo i14 out_coff */
  OMNI_OP_MAXPOOL = 3,
  /* nearest-neighbour resize (F.interpolate mode='nearest') of a channel slice,
   * either overwriting or accumulating into y (Upsample, CBFuse).
   *  p0 x p4 y; i0 B i1 H i2 W i3 C i4 ldi i5 in_coff i10 Ho i11 Wo i13 ldo i14 out_coff i18 accumulate
   *  i17 = n > 1 (CBFuse in one launch): y = ((r(x0) + r(x1)) + ...) over n <= 5 sources of C channels in order, r = nearest resize to
   *  Ho x Wo; source 0 as above, sources 1..4 = p1, p2, p3, p5 with (H, W, ld, coff) in i19-22, i23-26, i27-30, (i7, i12, i15, i16);
   *  the same partial sums, rounded the same way, as n launches with i18 = 1 */
  OMNI_OP_RESIZE_NEAREST = 4,
  /* Pillow-exact separable resample (LANCZOS/BICUBIC, 8bpc fixed point) +
   * letterbox + /255 -> network input.  Replaces ref:util/yolov9.py:73-87.
   *  p0 img u8 [H,W,3]  p1 tmp u8 [H,Wr,3]  p2 xbounds i32[Wr*2] p3 xcoef i32[Wr*kx]
   *  p5 ybounds i32[Hr*2] p6 ycoef i32[Hr*ky]  p4 y [1,TH,TW,ldo] (channels >=3 zeroed)
   *  i0 H i1 W i2 Hr i3 Wr i4 kx i5 ky i6 TH i7 TW i8 pad_left i9 pad_top i13 ldo
   *  i10 need_h i11 need_v (0 => that pass is a copy, Pillow's same-size shortcut) i12 batch index */
  OMNI_OP_LETTERBOX = 5,
  /* DFL expectation + anchor decode + sigmoid + max-class + threshold +
   * un-letterbox + compaction.  Replaces ref:util/yolov9.py:89-129.
   *  p0..p2 cls logits per stride [H_s*W_s, ldc_s]; p3..p5 box logits [H_s*W_s, ldb_s] (4*16 DFL bins, or 4 if i12==1)
   *  p6 cand (omni_cand_t[cap])  p7 count i32[1]
   *  i0 nc i1 TH i2 TW (network input size) i3..i5 ldc_s i6..i8 ldb_s i9 cap i10 pad_left i11 pad_top
   *  i12 dist_is_reduced i13..i15 cls channel offsets i16..i18 box channel offsets i19 batch index
   *  f0 conf f1 scale */
  OMNI_OP_DETECT_DECODE = 6,
  /* class-aware greedy NMS identical to torchvision.ops.batched_nms on CPU
   * (ref:util/yolov9.py:131) + [:max_det] + clamp (:134-135).
   *  p0 cand p1 count p2 sorted cand scratch (cap) p3 mask scratch u64[cap*ceil(cap/64)]
   *  p4 out boxes f32[max_det,4] p5 out scores f32[max_det] p6 out cls i32[max_det] p7 out count i32[1]
   *  i0 cap i1 max_det i2 img_w i3 img_h ; f0 iou
   *  i4 frames (0 = 1): frame f reads cand + f*cap records, count[f], sorted + f*(cap+1) records, writes out_* + f*max_det, out_count[f]
   *  (the mask scratch is shared: frames that need it run one after another); i5 = 1: force the tiled kernels (tests).
   *  Frames with <= 2048 candidates are sorted and suppressed by one workgroup out of LDS; the result is the same list either way.
   *  omni_cand_t.anchor (the tie-break of equal scores = torch's stable sort over anchor order) must lie in [0, 2^21) on that path —
   *  true of everything OMNI_OP_DETECT_DECODE writes; values outside are saturated (never mis-sorted against the score) and tie-break
   *  by slot.  A caller with larger anchor ids sets i5 = 1. */
  OMNI_OP_NMS = 7,
  /* x + depthwise3x3(x) + bias (DaViT conv1/conv2, hf:models/florence2/modeling_florence2.py:432-436).
   *  p0 x [B,H,W,C] p1 w [3][3][C] p2 bias f32[C] p4 y; i0 B i1 H i2 W i3 C */
  OMNI_OP_DWCONV3 = 8,
  /* nn.LayerNorm over C (<= 1024) of x (+ add[row % period]) (hf florence2 :154-574, bart :272-341).
   *  p0 x [rows,C] p1 add [period,C] or NULL p2 gamma f32 p3 beta f32 p4 y; i0*i1 rows i3 C i5 period; f0 eps
   *  i6 output mode (f32 plans, C % 16 == 0): 0 = f32 y, 1 = y in format B (see OMNI_OP_CONV i20 = 2), 2 = f32 y AND format B p5 */
  OMNI_OP_LAYERNORM = 9,
  /* softmax(q k^T * scale) v, one query row per thread; mode 0 plain MHA (bart :143-257), mode 1 DaViT
   * 12x12 window attention incl. the unmasked zero-padded window tokens (florence2 :338-398).
   *  p0 q p1 k p2 v (token matrices) p4 o p5 kbias f32 p6 vbias f32 (window padding rows)
   *  i0 ldq i1 ldk i2 ldv i3 ldo i4 qoff i5 koff i6 voff i7 ooff i8 heads i9 nq i10 nk i11 groups
   *  i12 mode i13 H i14 W i15 head_dim (32|64); f0 scale
   *  i16 = 1 (f32 plans, MFMA kernels): write o in format B (see OMNI_OP_CONV i20 = 2) for the LDS-DMA GEMM that follows
   *  f32 plans, MFMA kernels (mode 1 with head_dim 32, mode 0 with head_dim 64): row pitches and channel offsets % 4 == 0
   *  Ragged prompts (additive; NULL = all nk keys): p7 valid keys per group i32[groups], mode 0 only.  Group g attends to its first
   *  p7[g] keys (clamped to 1..nk); its rows still lie nk apart, so rows at or beyond the count exist and are only read as
   *  queries: they are computed over the valid keys, stay finite, and nobody reads them as keys. */
  OMNI_OP_ATTN_ROWS = 10,
  /* DaViT grouped channel attention (florence2 :223-259): p0 qkv [B*N,3C] p4 o [B*N,C] p5 ws f32[B*G*chunks*1024]
   *  i0 B i1 N i3 C i4 G i5 chunk_tokens i6 = 1: o in format B (f32 plans); f0 scale (0 => N^-0.5)
   *  i8 = 1 (additive; f32 plans, C % 64 == 0, i5 % 8 == 0): FOLD MODE.  The group's 32x32 matrix A_g = softmax(scale q^T k) does not
   *  depend on the token and the projection Wp behind the attention is linear, so proj(attn)[n][o] = sum_c W'_b[o][c] v[n][c] + bias with
   *  W'_b[o][g32+j] = sum_i Wp[o][g32+i] A_g[i][j].  The op computes scores and softmax as always, then W'_b per image instead of the
   *  apply pass: p1 Wp f32[C, C] (plain), p2 W' f32[B, C, C] (one fma chain per element, i ascending), p3 the same as format-B
   *  matrices [B][C][C] of 4 bytes per element with W' 2^k = hi + lo, k per image such that the largest |W' 2^k| lies in [2^12, 2^13)
   *  (clamped to +-24; 0 for a zero matrix), p6 f32[B] = 2^-k, p7 f32[B * (C / 64) * G] scratch (block maxima).  p4 is not written and
   *  may be NULL; q and k are read from p0 as f32, v is not read.  p3 / p6 feed OMNI_OP_CONV i26 / i27 / p6
   *  i9 = 1 (additive; f32 plans, i5 % 8 == 0): p5 ALREADY HOLDS THE PARTIALS [B][G][chunks][32][32] (written by OMNI_OP_CONV i28 = 1 with
   *  i5 = 256): the scores launch is skipped, p0 is not read; softmax (partials summed per element in ascending chunk order) and what
   *  follows run as always
   *  i10 = t > 0 (additive; f32 plans, t % 8 == 0, i5 % t == 0; 0 = i5): TOKENS PER PARTIAL.  Every chunk of i5 tokens is kept as i5 / t
   *  partials of t tokens: chunks = ceil(N / t) in the layout of p5, in the scores launch and in the softmax's sum — the op at i5 = t, bit
   *  for bit.  The captioner's folded stages run i5 = 1024, i10 = 256 (the row tile of OMNI_OP_CONV i28 = 1)
   *  i11 = 1 (fold mode only, additive; C % 128 == 0): Wv FOLDED IN AS WELL — the projection will read the block's LayerNorm output h,
   *  y = h . (W'_b Wv)^T + b''_b.  p1 = f32[C * C + 2 C]: Wp, then the v bias bv, then the projection bias bp.  p2 = f32[B * C * C + B * C]:
   *  W' as always, and behind the B matrices the bias table b''_b[o] = (sum_c W'_b[o][c] bv[c]) + bp[o], one fma chain per output over c
   *  ascending from 0, computed from the f32 W'_b.  f1 = 2^-kv of the packed Wv^T (0 => 1): p6[b] = 2^-k * f1 (exact), the scale of the fold
   *  GEMM (OMNI_OP_CONV i26 = C, i27 = 0) that overwrites p2's matrices with W''_b = W'_b . Wv; OMNI_OP_SPLIT_CONVERT i6 = 1 then re-packs
   *  them into p3 / p6, and the projection runs with OMNI_OP_CONV i29 = 1 on the table.  Everything else as i11 = 0, bit for bit */
  OMNI_OP_CHAN_ATTN = 11,
  /* projector input (florence2 :568-590): y[b] = [mean_n(x+pos+t) ; x+pos+t]; p0 x [B,N,C] p1 pos2d f32[N,C] p2 temporal f32[C] p4 y [B,N+1,C]
   *  i0 B i1 N i3 C */
  OMNI_OP_PROJ_PREP = 12,
  /* encoder input = [image features ; prompt embeddings] (florence2 :933-960): p0 img [B,n_img,C] p1 txt [n_txt,C] p4 y
   *  i0 B i1 n_img i2 n_txt i3 C
   *  Prompt as a plan input (additive; p2 NULL = the constant block p1): p2 ids i32[B,n_txt] p3 token table [i4, C] (plan dtype),
   *  p1 NULL; y[b][n_img + t] = table[ids[b][t]] * f0 (0 => 1).  Positions behind a row's prompt hold the pad token.  The caller
   *  checks 0 <= id < i4 before it writes the ids; the kernel clamps. */
  OMNI_OP_ASSEMBLE = 13,
  /* decoder token embedding + learned position (bart :80-98): y[b] = table[ids[b][step]]*scale + pos[step+off]
   *  p0 table p1 pos p2 ids i32[B,T] p4 y [B,C] p6 step i32*; i0 B i3 C i4 T i5 pos offset; f0 scale */
  OMNI_OP_EMBED_STEP = 14,
  /* single-query attention, head_dim 64: self (append k/v at `step` to the cache, attend 0..step) or cross
   * (nk_fixed keys).  p0 q p1 knew p2 vnew p3 kcache [B,cap,C] p5 vcache p4 o [B,ldo] p6 step
   *  i0 ldq i1 qoff i2 ldn i3 koff i4 voff i5 ldo i6 heads i7 nk_fixed i8 cap i9 C i10 B i11 cache row stride (0 => C); f0 scale
   *  Beam plans (additive; NULL / 0 = the behaviour above): p7 self-attention position table i32 [B, cap], entry [b][t] = the
   *  cache row that holds position t of row b (row b still appends its own k / v at (b, step)); i12 cross-attention rows per
   *  cache row: row b reads kcache / vcache row b / i12 (the k beams of a crop share its one cross-K / V row)
   *  Ragged prompts (additive; NULL = nk_fixed keys everywhere): in cross-attention (i7 > 0, which needs i7 <= i8) p7 is the
   *  number of valid keys per cache row, i32[ceil(B / i12)], read at b / i12 and clamped to 1..nk_fixed
   *  Which kernel launches (same slots, same result up to summation order): cross-attention of f32 plans with i0, i1, i11 % 4 == 0
   *  -> attn_decode_cross_kernel (four waves per (row, head), four keys per 16-byte load).  Self-attention (i7 <= 0) of f32 plans
   *  without a position table, with i8 (cap) > 64 and i0, i1, i2, i3, i4, i11 % 4 == 0 -> attn_decode_self_kernel, the same mapping on
   *  keys 0..step; the step's own key / value are taken from p1 / p2, never read back from the cache row appended in the same launch,
   *  and cache rows beyond `step` are never read.  Everything else (cap <= 64, f16 plans, beam plans, unaligned pitches) -> the generic
   *  one-wave kernel, which is correct at any cap. */
  OMNI_OP_ATTN_DECODE = 15,
  /* greedy decoding step (hf:generation/utils.py:2783-2937 + logits_process NoRepeatNGram/ForcedBOS/ForcedEOS):
   *  p0 logits [B,ldl] p1 final_logits_bias f32 or NULL p2 ids i32[B,T] p3 finished i32[B] p6 step i32*
   *  i0 B i1 vocab i2 ldl i3 T i4 max_new_tokens i5 no_repeat_ngram i6 bos i7 eos i8 pad i9 forced_bos(-1)
   *  i10 forced_eos(-1) i11 increment step afterwards
   *  Which kernel launches (same slots, same semantics): greedy_step_kernel keeps the tokens banned by NoRepeatNGram in a list of 32,
   *  which a history of i4 tokens cannot overflow while i4 - i5 + 1 <= 32 (the n-gram start positions of a full history); with
   *  i5 > 0 and i4 - i5 + 1 > 32 greedy_step_long_kernel launches instead: the bans go into a bitmap over the vocabulary in LDS
   *  (((i1 + 31) / 32 + i3) x 4 bytes <= 48 KiB, else OMNI_E_ARG), exact for any history up to T.  Forced tokens, bias, the
   *  lowest-index tie rule, id 0 for a row without a finite logit, pad for finished rows and p4 are those of greedy_step_kernel, and
   *  both give bit-identical results on a history the list can hold.  The target-score form (p5) has no ban and one kernel.
   *  Token scores (additive; p4 NULL = the kernel above, nothing else computed): p4 f32 [B, T] token log-probabilities.  The step that
   *  writes ids[b][st + 1] also writes p4[b][st + 1] = log_softmax(processed scores)[id] — processed = logits + bias with the
   *  NoRepeatNGram bans at -inf, i.e. transformers' compute_transition_scores(normalize_logits=True) of its greedy `scores` —
   *  accumulated in f32 for both logit types; 0 at a forced position (hf's processed row is 0 there and -inf elsewhere) and for a row
   *  that had finished before the step (it emits pad).  Column 0 (the start token) is never written.  ids, finished and step are
   *  bit for bit what p4 = NULL writes.  A row without a finite logit (id 0) gets an unspecified value.
   *  Target scores (additive; p5 NULL and p7 NULL = the forms above): a non-NULL p5 turns the step from choosing a token into
   *  SCORING a given one (teacher forcing) under the RAW model distribution — p5 tlen i32 [B] target lengths, p7 top1 i32 [B, T] or
   *  NULL, p4 required (p5 with p4 NULL, or p7 without p5: OMNI_E_ARG), p3 neither read nor written (may be NULL), i4 and the
   *  processors i5 (n-gram ban), i9 (forced bos), i10 (forced eos) ignored, i11 as above.  Row b reads tok = ids[b][st + 1] and never
   *  writes ids.  If st + 1 <= tlen[b]: p4[b][st + 1] = log_softmax(logits[b] + bias)[tok], accumulated in f32 in ONE pass over the
   *  row (online maximum / rescaled sum), and p7[b][st + 1] = the row's arg-max (lowest index among equals; 0 for a row without a
   *  finite logit, as above); otherwise both entries stay as they are (the host zeroes them).  A tok outside 0..vocab-1 scores -inf
   *  and reads nothing outside the row; a target whose logit is -inf scores -inf, never NaN. */
  OMNI_OP_GREEDY_STEP = 16,
  /* crop -> cv2.resize 64x64 INTER_LINEAR -> [Pillow BICUBIC to RxR] -> rescale, normalise
   * (ref:util/utils.py:97-105,120-123 + hf CLIP image processor).
   *  p0 img u8 [H,W,3] p1 boxes i32[n,4] (x0,y0,x1,y1 px) p2 c64 u8[n,64,64,3] p3 tmp u8[n,64,R,3]
   *  p4 y [n,R,R,ldo] p5 bounds i32[R,2] p6 coef i32[R,ksize] p7 lut f32[256]
   *  i0 n i1 H i2 W i3 R i4 ksize i13 ldo; f0..2 mean f3..5 std */
  OMNI_OP_CROP_RESIZE = 17,
  /* fused x1 = x + depthwise3x3(x) + bias ; h = LayerNorm(x1) (DaViT half-block prologue, hf florence2 :432-441).
   *  p0 x [B,H,W,C] p1 w [3][3][C] p2 bias f32[C] p3 h [B,H,W,C] p4 x1 [B,H,W,C] p5 gamma f32 p6 beta f32
   *  i0 B i1 H i2 W i3 C (<= 1024) i6 = 1: h in format B (f32 plans); f0 eps */
  OMNI_OP_DWCONV3_LN = 18,
  /* f32 channel slice of a token matrix -> format B (OMNI_OP_CONV i20 = 2), in place when p0 == p4 and the slices coincide.
   *  p0 x [rows, ldi] p4 y [rows, ldo]; i0*i1 rows i3 C i4 ldi i5 in_coff i13 ldo i14 out_coff (all multiples of 16)
   *  i6 = 1 (additive; f32 plans): PER-MATRIX POWER OF TWO.  p0 = i0 square f32 matrices [C][C] (i1 = i3 = i4 = i13 = C, C % 64 == 0,
   *  i5 = i14 = 0), each packed as format B of x * 2^k with k per matrix such that the largest |x 2^k| lies in [2^12, 2^13) (clamped to
   *  +-24; 0 for a zero matrix; hi and lo rounded to nearest) — the packing OMNI_OP_CHAN_ATTN's fold mode gives W'_b, here for the W''_b
   *  of a block with Wv folded in.  p6 = f32[i0] receives 2^-k, p5 = f32[i0 * (C / 64) * (C / 32)] scratch (block maxima: no atomics,
   *  nothing to zero between replays) */
  OMNI_OP_SPLIT_CONVERT = 19,
  /* Detect -> caption hand-off of ONE screenshot on the device: ref:util/utils.py:432-453 (ratio boxes, int_box_area filter),
   * remove_overlap_new (:241-319, incl. its list.remove quirk), the "content is None last" ordering (:449-451) and the crop
   * rectangles of get_parsed_content_icon (:90-98), in the reference's own mix of f32 / Python-float (f64) arithmetic.
   *  p0 boxes f32[max_det,4] (px, score order; ratios if i5) p1 box count i32* p2 OCR boxes f64[cap,4] (ratios, already
   *  int_box_area-filtered by the host) p3 OCR table i32[2 + 2*cap]: {live OCR count, 0, (equality class, rank in class) per box}
   *  p4 out element table i32[i6,2]: (kind 0 OCR | 1 icon with OCR text | 2 icon to caption, source index) in output order
   *  p5 out crop rectangles i32[max_det,4] (x0,y0,x1,y1 px, caption order) p6 out i32[4]: {elements, crops, index of the
   *  first caption-less element or -1, surviving OCR boxes} p7 out donor bit masks u64[max_det, i4] (OCR boxes whose text an
   *  icon collects)
   *  i0 max_det (<= 512) i1 OCR capacity (<= 1024) i2 W i3 H i4 mask words per icon i5 boxes are ratios i6 element capacity
   *  i7 = 1: the overlap threshold is the f64 with bit pattern i9:i8 (Python passes 0.7 as a double), else f0 */
  OMNI_OP_GLUE = 20,
  /* Set-of-marks overlay rastered in place on the device (ref:util/utils.py:478-483 annotate() -> ref:util/box_annotator.py:86-162;
   * the draw list comes from util/overlay.py::plan_overlay, pinned to the reference's cv2 call sequence): painter's algorithm over
   * a primitive list, in order.  p0 frame u8[H,W,3] (in / out) p1 primitives i32[n,8] = {kind, x0, y0, x1, y1, r | g<<8 | b<<16,
   * a, 0}: kind 0 filled rectangle (x1, y1 inclusive), 1 ring = the pixels of the rectangle that are not in its interior shrunk by
   * a = width on every side, 2 coverage mask (x1, y1 exclusive; a = byte offset of its (y1-y0) x (x1-x0) u8 mask in p2) blended
   * like Pillow's draw_bitmap; p2 masks u8.  i0 H i1 W i2 n
   *  Frame batch (additive; p3 = p4 = NULL and i3 = 0: the in-place form above): ONE launch over i3 = B >= 1 equal-sized frames, OUT OF
   *  PLACE — p0 destination u8[B,H,W,3], every pixel of it is written (the source value where nothing draws; a frame without
   *  primitives is a copy); p3 device table of B source frame pointers (u8[H,W,3] each, never written, may not overlap p0);
   *  p1 the primitive lists of all frames one after the other, i2 their total; p4 i32[B + 1] offsets: frame f draws primitives
   *  p4[f] .. p4[f + 1]; p2 ONE mask blob, the `a` of a kind-2 primitive is its ABSOLUTE byte offset in it.  Either of p3 / p4 / i3
   *  set selects this form, and then a NULL p3 / p4 or B < 1 is OMNI_E_ARG */
  OMNI_OP_OVERLAY = 21,
  /* Frame -> PNG file -> base64, all on the device (ref:util/utils.py:485-488: PIL save(format="PNG") + base64.b64encode):
   * signature, IHDR (8-bit RGB), ONE IDAT whose zlib stream holds stored deflate blocks (filter 0 scanlines; 65535-byte blocks),
   * IEND; Adler-32 and the chunk CRC-32 are computed on the device.  File size = H (3 W + 1) + 5 ceil(H (3 W + 1) / 65535) + 63.
   *  p0 frame u8[H,W,3] p1 out PNG bytes p2 scratch u32[2 H + ceil((size - 53) / 4096)] p3 out base64 ASCII (4 ceil(size / 3)
   *  bytes) or NULL.  i0 H i1 W i2 scratch words i3 capacity of p1 in bytes (0 = not checked) */
  OMNI_OP_PNG_PACK = 22,
  /* Same file as OMNI_OP_PNG_PACK with a COMPRESSED zlib stream (size known only on the device): scanlines Up-filtered (row 0:
   * None), the filtered stream cut into 4096-byte units, each unit ONE fixed-Huffman deflate block of literals and run matches
   * (distance 1 / 3) + an empty stored block (byte alignment), or one stored block when that is not smaller — one GPU thread per
   * unit, then offsets, gather, Adler-32, CRC-32, base64 as above.  Worst case = the stored size with 4096-byte blocks.
   *  p0 frame u8[H,W,3] p1 out PNG bytes (capacity i2) p2 scratch: filtered stream u8[H (3 W + 1)] p3 scratch: unit slots
   *  u8[units * 4640] p4 out/scratch meta u32[i3]: {zlib stream bytes, FILE BYTES, base64 bytes, CRC segments, unit sizes..., unit
   *  offsets...} p5 scratch u32[i4] (Adler / CRC partials) p6 out base64 ASCII (4 ceil(capacity / 3) bytes) or NULL
   *  i0 H i1 W i2 capacity of p1 (>= H (3 W + 1) + 5 units + 63) i3 meta words (>= 4 + 2 units) i4 scratch words
   *  (>= 2 H + ceil((capacity - 53) / 4096))
   *  i5 = 1 (round 6, what `OMNI_OVERLAY=device` uses): LZ77 + DYNAMIC Huffman instead — units of 32768 bytes, one GPU lane per
   *  unit: greedy matches against distance 1 / 3 and a 13-bit single-entry hash table of the unit's own 3-byte strings, one dynamic
   *  block per unit (length-limited canonical codes built on the device) + the empty stored block; ~1.1x (desktop screenshots) ...
   *  1.3x (noise-heavy frames) the bytes of Pillow's zlib level 6 (the fixed-Huffman variant: 2.7x).  Needs p3 >= ceil(H (3 W + 1) /
   *  32768) * 33792 bytes and p7 = token scratch u32[ceil(H (3 W + 1) / 32768) * 32768]; same capacities otherwise.  Bytes =
   *  oracle/png_ref.py::deflate_png_lz.
   *  i5 = 2 (additive): the i5 = 1 stream for i6 = B >= 1 equal-sized frames in the SAME nine launches (frame = a grid dimension;
   *  the per-unit encoder is the same code, so every file is deflate_png_lz of its frame).  p0 u8[B,H,W,3]; p1..p7 hold B parts one
   *  after the other, each of the per-frame capacity of the i5 = 1 form: p1 [B][i2] p2 [B][H (3 W + 1)] p3 [B][units * 33792]
   *  p4 [B][i3] p5 [B][i4] p6 [B][4 ceil(i2 / 3)] or NULL p7 [B][units * 32768]; i2 / i3 / i4 stay PER-FRAME capacities with the
   *  same lower bounds.  B < 1 is OMNI_E_ARG.  i6 is ignored unless i5 = 2; the fixed-Huffman variant has no batched form */
  OMNI_OP_PNG_DEFLATE = 23,
  /* FFN of a DaViT block as one kernel (hf:models/florence2/modeling_florence2.py Florence2VisionMLP inside the residual of
   * Florence2VisionSpatialBlock / ChannelBlock): y = residual + fc2(GELU(fc1(x))), hidden activations kept in registers
   * (csrc/gemm_dma.hip::mlp_fused_kernel).  f32 plans, C = 128, hidden = 512 (DaViT stage 0 of Florence-2-base).
   *  p0 x [rows, ldi] in format B (see OMNI_OP_CONV i20 = 2)   p1 w1 format B [hidden][C], = split(W1 * 2^k1)   p2 b1 f32[hidden]
   *  p3 residual f32 [rows, ldr]   p4 y f32 [rows, ldo] (may alias the residual)   p6 b2 f32[C]
   *  p5 w2 format B [C][hidden] = split(W2 * 2^k2) with the hidden axis permuted inside every 16-group to
   *     {0,1,2,3, 8,9,10,11, 4,5,6,7, 12,13,14,15} (the order in which the first product's accumulators hold it)
   *  i0*i1 rows i3 C i4 ldi i5 in_coff i12 hidden i13 ldo i14 out_coff i16 ldr i17 res_coff; f1 2^-k1 f2 2^-k2 */
  OMNI_OP_MLP_FUSED = 24,
  /* beam-search decoding step, transformers' _beam_search (hf:generation/utils.py:3008-3523): per crop (one workgroup), k beams
   * = decoder rows [b k, b k + k): log_softmax(logits + final_logits_bias) in f32, NoRepeatNGram / ForcedBOS / ForcedEOS on the
   * log-probs, + running score, top-2k over k x V, next running beams, finished-beam merge with the length penalty, early-stop
   * heuristic; the crop's rows of p2 / p4 / p5 are reordered in place.  A frozen crop (heuristic satisfied, early_stopping True
   * with k finished entries, or all 2k candidates stopped) is left as it is.  Ties: lower flat index first.
   *  p0 logits [B k, ldl] p1 final_logits_bias f32 or NULL p2 running ids i32[B k, T] p3 running scores f32[B k]
   *  p4 self-attention position table i32[B k, T] (OMNI_OP_ATTN_DECODE p7) p5 finished ids i32[B, k, T] p6 step i32*
   *  p7 state, 4-byte words: finished scores f32[B, k] | finished flags i32[B, k] | finished lengths i32[B, k] (generated tokens)
   *     | heuristic unsatisfied i32[B] | frozen i32[B]
   *  i0 B (crops) i1 vocab i2 ldl i3 T i4 max_new_tokens i5 no_repeat_ngram i6 k (2..8) i7 eos i8 pad i9 forced_bos(-1)
   *  i10 forced_eos(-1) i11 increment step afterwards i12 early_stopping (0 False, 1 True, 2 "never"); f0 length_penalty.
   *  3 k T * 4 bytes of LDS <= 48 KB.  The model-level entry points (omni_captioner_*) and plan bundles stay greedy.
   *  Value 25: the next enumerator after OMNI_OP_MLP_FUSED (implicit, so the explicitly numbered kinds 1..24 stay the list they were). */
  OMNI_OP_BEAM_STEP,
  OMNI_OP__COUNT,   /* = 26: one past the implicitly numbered kinds above.  Kinds added since follow with explicit values (this line
                     * stays directly behind OMNI_OP_BEAM_STEP, where callers and tests expect it); OMNI_OP__END is one past the last kind */
  /* greedy decoding step WITH GENERATION CONTROLS: OMNI_OP_GREEDY_STEP's generating form (p0..p6 and i0..i11 mean exactly what they
   * mean there, p4 = token log-probabilities included; p5 must be NULL: there is no target-score form) plus the deterministic
   * logits processors a transformers caller sets per call, read from DEVICE memory at run time — one captured step graph serves
   * every setting, nothing is baked into a plan:
   *  p7 control block (layout below, 4-byte aligned)   i12 its size in bytes
   * Per row, in transformers' order (generation/utils.py _get_logits_processor), on x = logits + final_logits_bias in f32:
   *  1 RepetitionPenalty: every token that occurs in ids[b][0..st] (the decoder start token included), once however often it
   *    occurs: x < 0 ? x * penalty : x / penalty (f32, IEEE divide)
   *  2 NoRepeatNGram with the block's n-gram size; -1 = the op's i5 (the checkpoint's value), 0 = off
   *  3 NoBadWords: entry [t0..tk] (k >= 1) puts tk at -inf when k + 1 <= st + 1 and the last k tokens of the history equal t0..tk-1
   *    (single-token entries are folded into the suppress bitmap by the host)
   *  4 MinNewTokensLength: eos (i7) at -inf while st < min_new_tokens
   *  5 ForcedBOS / ForcedEOS as in OMNI_OP_GREEDY_STEP (the forced token, log-probability 0)
   *  6 SuppressTokens: the suppress bitmap, at every step
   *  7 SuppressTokensAtBegin: the begin-suppress bitmap at st + 1 == begin_index only
   * then the arg-max (lowest index among equals), id 0 for a row without a finite entry, pad for finished rows, the EOS bookkeeping
   * and, with p4, log_softmax(processed)[id] in a second pass that recomputes the same processed values.
   * Control block, 4-byte words (struct omni_gen_ctrl is the header):
   *  word 0 f32 repetition penalty (1.0 = none)   1 i32 n-gram size (-1 = i5)   2 i32 min_new_tokens   3 i32 begin_index
   *  4 i32 n = number of bad-word sequences (0..OMNI_GEN_CTRL_MAX_BAD)   5 i32 stride = words per sequence, 1 + Lmax with
   *  Lmax <= OMNI_GEN_CTRL_MAX_BAD_LEN (0 when n = 0)   6, 7 reserved (0)
   *  then u32[W] suppress bitmap, u32[W] begin-suppress bitmap, W = (i1 + 31) / 32 (bit v & 31 of word v >> 5 = token v),
   *  then i32[n][stride] bad-word table, every row {length L (2..Lmax), t0 .. tL-1, unused}.
   * i12 >= 32 + 8 W + 4 n stride, with n and stride as the header in p7 holds them when omni_op_launch / omni_plan_create see the
   * op (they read the 32-byte header back), else OMNI_E_ARG; with the pointer check on, p7 + i12 lies inside one allocation.  The
   * kernel itself never reads beyond i12 bytes whatever the block says later: sequences that do not fit are not read.
   * One kernel, greedy_ctrl_step_kernel, always: the bitmap (long-history) form of the n-gram ban — the n-gram size is not known
   * when the op is recorded — with a second bitmap of the tokens seen.  LDS: (2 W + i3 + 64) x 4 bytes + the reduction arrays
   * <= 48 KiB, else OMNI_E_ARG (17 KB at a vocabulary of 51289 and T = 1025).  A neutral block (penalty 1.0, n-gram -1, nothing else
   * set) gives bit for bit what OMNI_OP_GREEDY_STEP gives.  Value 26; plan bundles and the model-level entry points do not use it. */
  OMNI_OP_GREEDY_CTRL_STEP = OMNI_OP__COUNT,   /* 26, the number the end mark of the list above has */
  /* greedy decoding step over a CLOSED VOCABULARY: OMNI_OP_GREEDY_STEP's generating form (p0..p4, p6 and i0..i11 mean exactly what
   * they mean there, p4 = token log-probabilities or NULL) with transformers' PrefixConstrainedLogitsProcessor for a fixed set of
   * labels: the set is a trie in DEVICE memory, read at every step — one captured step graph serves every vocabulary.
   *  p5 node i32[B], read and written: the row's trie node, 0 = root (the caller zeroes it before the first step), -1 = left the trie
   *  p7 trie block (layout below, 4-byte aligned)   i12 its size in bytes
   * Per row, in transformers' order (generation/utils.py _get_logits_processor): NoRepeatNGram (i5; exact for any history),
   * PrefixConstrained, ForcedBOS, ForcedEOS — x = logits[tok] + final_logits_bias[tok] in f32 is taken ONLY at the edge tokens of
   * node[b]; nothing else of the row's logits is read.  Edges whose token the n-gram ban of ids[b][0..st] hits are at -inf.  Then the
   * arg-max (lowest token id among equals), or the forced token at a forced position; pad for finished rows and the EOS bookkeeping
   * of OMNI_OP_GREEDY_STEP; with p4, log_softmax over the allowed, unbanned children at the token — exactly 0.0 at a forced
   * position, for a finished row and at a node with one allowed child.  node[b] becomes the child the emitted token leads to (the
   * forced token moves it too), -1 when no edge of the node carries that token; finished rows leave it alone.  A row at node -1, at a
   * node without edges, or whose edges are all -inf / NaN emits id 0 (its log-probability is unspecified), as the other greedy
   * kernels do for a row without a finite entry.
   * Trie block, 4-byte words, CSR (struct omni_vocab_trie is the header):
   *  words 0..7 {n_nodes (1..OMNI_VOCAB_MAX_NODES), n_edges, longest label in tokens, 0, 0, 0, 0, 0}
   *  then first i32[n_nodes + 1] (edges of node k = [first[k], first[k + 1])), edge_tok i32[n_edges] (ascending within a node),
   *  edge_dst i32[n_edges] (the child node).  Node 0 is the root; in a trie n_edges = n_nodes - 1.
   * i12 >= 32 + 4 (n_nodes + 1 + 2 n_edges), with n_nodes and n_edges as the header in p7 holds them when omni_op_launch /
   * omni_plan_create see the op (they read the 32-byte header back), else OMNI_E_ARG; with the pointer check on, p7 + i12 lies inside
   * one allocation.  The kernel itself never reads beyond i12 bytes whatever the block says later: the header's counts are clamped
   * to i12, edge ranges to the edge arrays, and edge tokens outside 0..i1-1 are skipped.
   * One kernel, greedy_vocab_step_kernel (csrc/vocab_step.hip).  LDS: i3 x 4 bytes + the reduction arrays <= 48 KiB, else
   * OMNI_E_ARG.  Plan bundles and the model-level entry points do not use it. */
  OMNI_OP_GREEDY_VOCAB_STEP = OMNI_OP_GREEDY_CTRL_STEP + 1,   /* 27 (spelled like the kind above: the literally numbered kinds stay 1..24) */
  /* VISUAL EMBEDDINGS of crops and exemplar matching (csrc/visual_match.hip).  Row 0 of a crop's img_feat — the spatial-average
   * token behind image_projection and image_proj_norm — is Florence-2's global descriptor of the crop.  i0 selects the mode:
   *  i0 = 0, embed (embed_rows_kernel, one wave per crop):
   *    p0 x [i1 rows of i2 elements] of the op's dtype (f32 / f16): the first i3 elements of a row are read   p4 y f32[i1, i3]
   *    p5 norm f32[i1]        i1 = crops (1..65536)  i2 = row stride in elements (n_img D; % 4 == 0, >= i3)  i3 = D (% 4 == 0, <= 4096)
   *    y = x / |x| with |x| accumulated in f32; a zero row gives a zero vector and norm 0.  p0 / p4 aligned to 4 elements.
   *  i0 = 1, partial top-k (match_partial_kernel):
   *    p0 Q f32[i1, i3] and p1 G f32[i2, i3], unit vectors, 16-byte aligned   p5 partials, 8-byte aligned   i6 = bytes of p5
   *    i1 = m queries (1..4096)  i2 = n gallery rows (1..65536)  i3 = D (% 4 == 0, <= 4096)  i4 = k (1..8)
   *    i5 = gallery rows per split, 0 = the launcher's choice (a large gallery fills the chip, a small one is one block per group
   *    of 8 queries); a value > 0 is the test handle, as the conv op's tile override i22 is.
   *    Grid (splits, groups of 8 queries).  The score of (q, g) is the f32 dot product in one summation order that depends on D
   *    alone: the same bits under every i5.  p5 receives {f32 score, i32 gallery index} [m][splits][k], each query's best k of
   *    each split, -inf / -1 where a split has fewer rows.
   *  i0 = 2, merge (match_merge_kernel), a second launch with the same i1..i6 and p5:
   *    p4 idx i32[m, k]   p6 score f32[m, k]: descending score, the lower gallery index first among equals; positions behind
   *    min(k, n) hold -1 and -inf.
   * OMNI_E_ARG (nothing launched, nothing written): any value outside its range, a NULL or misaligned pointer, i6 below the
   * m x splits x k x 8 bytes of the split in force (omni_visual_match_cfg reports them).  The pointer check covers exactly those
   * extents.  The op's dtype matters to mode 0 only.  Plan bundles and the model-level entry points do not use it. */
  OMNI_OP_VISUAL_MATCH = OMNI_OP_GREEDY_VOCAB_STEP + 1,   /* 28 (spelled like the two kinds above) */
  /* REGION OCR: Florence-2's <OCR_WITH_REGION> task over native-resolution tiles of a screenshot (csrc/region_ocr.hip).  i0 selects
   * the mode:
   *  i0 = 0, tile cut (tile_cut_kernel, one work-item per tile pixel):
   *    p0 frame u8[i2, i3, 3] (H, W)   p1 origins i32[i1, 2] {x, y} of the tiles' top-left pixels in the frame, any sign
   *    p4 y [i1][i4][i4][i13] of the op's dtype (f32 / f16): a caption plan's input, the layout, pitch and zeroed padding channels
   *    OMNI_OP_CROP_RESIZE writes   p7 f32[256], f32(f64(u8) * (1/255))   f0..f2 mean, f3..f5 std (not 0)
   *    i1 = tiles (1..65536)  i4 = R (1..65536)  i13 = elements per pixel (3..64)
   *    y = (p7[u8] - mean) / std in f32, stored in the op's dtype: the image processor with do_resize = False.  A tile pixel outside
   *    the frame takes u8 255 on all channels first (the tile pasted on a white canvas); the frame is never read outside.
   *  i0 = 1, region parse (region_parse_kernel, one 64-lane block per row):
   *    p0 ids i32[i1 rows, stride i5 (0 = i2)]: column 0 the decoder start token, then the generated tokens   i2 = T (2..2049)
   *    p1 class table u16[i4]: 0..999 = location bin, OMNI_OCR_CLASS_STRIP (<s>, </s>, <pad>: deleted before matching),
   *    OMNI_OCR_CLASS_TEXT, OMNI_OCR_CLASS_HARD (decoded text empty or holding a newline or '<'); larger values and ids outside
   *    0..i4-1 count as HARD   p2 logp f32[i1 rows, stride i6 (0 = i2 - 1)] aligned with ids[1:], or NULL
   *    p7 cells i32[i1, 6] per row {origin x, origin y, lo x, hi x, lo y, hi y}: the tile's origin in the frame and the cell it owns
   *    in DOUBLED frame pixels, lo inclusive, hi exclusive, INT_MAX = no upper end (origins within +-2^30)
   *    i3 = M, region slots per row: exactly (T - 1) / 9   i7 = R (1..65536)   i8 = the EOS id
   *    A row is columns 1 .. in front of the first EOS behind column 0 (all of them without one); nothing behind reaches an output.
   *    On its non-STRIP tokens, from p = 0: e = the smallest index >= p + 1 whose tokens e .. e + 7 are all location bins; region =
   *    content [p, e) (it may hold stray location tokens) + the eight bins; p = e + 8; until no e exists.  Corner q of a region is
   *    ((2 bin + 1) R) / 2000 + origin (x for even q, y for odd q).
   *    p4 records i32[i1 x M, 16], region k of row r at slot r M + k: {r, first and one-past-last ORIGINAL column of the content's
   *    non-STRIP tokens, x0 y0 .. x3 y3 in frame pixels, n = non-STRIP tokens of content + 8, kept, 0, 0, 0}; kept = the doubled
   *    centre (min + max over the four corners, per axis) lies in the row's cell on both axes.  Unused slots are zero.
   *    p5 sums f32[i1 x M]: logp over exactly those n tokens, added in ascending column order (0 with p2 = NULL and in unused slots)
   *    p6 rows i32[i1, 4] {regions found, regions kept, flags, 0}; flags bit 0 = the row holds a HARD token (the host re-parses
   *    it from text), bit 1 = no EOS in the generated part (cut off at max_new_tokens).
   *  i0 = 3, box parse (region_boxes_kernel, one 64-lane block per row): the answers of the tasks that reply "phrase <loc>x4 ..."
   *    (<OD>, <DENSE_REGION_CAPTION>, <OPEN_VOCABULARY_DETECTION>, <CAPTION_TO_PHRASE_GROUNDING>: grammar 0) or boxes alone
   *    (<REGION_PROPOSAL>: grammar 1).  Slots, the row, the classes, the cells and the flags as in mode 1, except:
   *    i3 = M, box slots per row: exactly (T - 1) / 4   i9 = grammar, 0 = phrases with boxes, 1 = boxes only
   *    The row's non-STRIP tokens are cut into alternating maximal runs: a text run [t, a) (classes >= 1000; empty only at the
   *    row's start), then a run of r location bins [a, a + r).  carry = none.
   *    grammar 1: a run with r >= 4 gives r / 4 boxes, four bins each from a, and an empty phrase.
   *    grammar 0: start = carry if there is one, else t if the text run is not empty, else none.  start and r >= 4: a phrase with
   *    content [start, a), lead = (start is the carry), r / 4 boxes from a; carry = none.  No start and r >= 5: a phrase that is the
   *    single token a, lead = 1, (r - 1) / 4 boxes from a + 1; carry = none.  Otherwise carry = the run's last token.  lead: the
   *    phrase's first token is a location token whose text counts WITHOUT its first character (transformers' pattern
   *    [^<]+(<loc_n>){4,} starts behind the '<' of a location token no earlier match consumed).  r mod 4 left-over bins are ignored.
   *    p4 records i32[i1 x M, 16], box k of row r at slot r M + k: {r, c0, c1, x0, y0, x1, y1, cloc, n_content, kept, phrase, lead,
   *    0, 0, 0, 0}: c0 / c1 the ORIGINAL columns of the phrase's first and one-past-last non-STRIP token (c0 = c1 = cloc in grammar
   *    1), corners ((2 bin + 1) R) / 2000 + origin, cloc the original column of the box's first location token, n_content the
   *    phrase's non-STRIP tokens, phrase its ordinal in the row (the boxes of one phrase share it), kept = (x0 + x1, y0 + y1) lies in
   *    the row's cell on both axes.  Unused slots are zero.
   *    p5 sums f32[i1 x M, 2] {logp over the phrase's n_content tokens, logp over the box's four location tokens}, each added in
   *    ascending column order (0 with p2 = NULL and in unused slots)
   *    p6 rows i32[i1, 4] {boxes found, boxes kept, flags, phrases found}
   *  i0 = 5, polygon parse (region_polys_kernel, one 64-lane block per row): the answers of the segmentation tasks
   *    (<REFERRING_EXPRESSION_SEGMENTATION>, <REGION_TO_SEGMENTATION>), transformers' "polygons" post-processing with
   *    allow_empty_phrase.  The row, the cells, the flags, p0 .. p2 and i4 .. i8 as in mode 1, except:
   *    i2 = T (3..2049)   i3 = P, polygon slots per row: exactly T / 2   i9 = V, vertex slots per row: exactly (T - 1) / 2
   *    classes: OMNI_OCR_CLASS_SEP (<sep>), OMNI_OCR_CLASS_POLY (<poly>) and OMNI_OCR_CLASS_POLY_END (</poly>) count here (modes 1
   *    and 3 take them as HARD); values above OMNI_OCR_CLASS_POLY_END and ids outside 0..i4-1 count as HARD.
   *    STRUCTURE tokens are the location bins, SEP, POLY and POLY_END.  A run is a maximal sequence of at least 4 structure tokens of
   *    the row's non-STRIP tokens (TEXT and HARD only separate runs); shorter sequences give nothing.  A run gives nothing unless a
   *    location bin or POLY stands in it, looking behind ONE leading location bin when it starts with one.  A run that holds both POLY
   *    and POLY_END gives the instances POLY content POLY_END, left to right without overlap: the first POLY, up to the next POLY_END,
   *    on behind it (no such pair: nothing); any other run is one instance whose content is the run.  In a content, every maximal
   *    sequence of location bins that SEP follows or that ends the content is a polygon (one that POLY or POLY_END follows is not);
   *    an odd number of bins drops the last, so a polygon may have 0 vertices; an instance without a polygon is dropped and not
   *    counted.  Vertex q of a polygon is ((2 bin + 1) R) / 2000 + origin from bins 2q (x) and 2q + 1 (y).
   *    p3 vertices i32[i1, V, 2] {x, y} in frame pixels: the row's vertices in answer order, polygon after polygon; unused slots zero
   *    p4 records i32[i1 x P, 16], polygon k of row r at slot r P + k: {r, instance ordinal, polygon ordinal within the instance, v0,
   *    nv, c0, c1, n_loc, kept, run ordinal, bx0, by0, bx1, by1, 0, 0}: v0 the polygon's first vertex slot, nv its vertices, c0 / c1 the
   *    ORIGINAL columns of its first location token and one past its last (a dropped odd one included), n_loc its location tokens,
   *    run the ordinal of its run among the row's runs, bx0 .. by1 the bounding box over ALL vertices of the instance (zeros without
   *    one), kept = the instance has a vertex and (bx0 + bx1, by0 + by1) lies in the row's cell on both axes.  Unused slots are zero.
   *    p5 sums f32[i1 x P]: logp over the 2 nv tokens that made the polygon's vertices, added in ascending column order (0 with p2 =
   *    NULL and in unused slots)
   *    p6 rows i32[i1, 4] {polygons found, instances found, flags, instances kept}
   *  i0 = 6, mask raster (poly_mask_kernel, one wave per pixel row, four pixel rows per block): mode 5's outputs, read where it left
   *    them, become bit masks.  i1 = rows  i2 = T as in mode 5 (P and V follow from it)  i3 = I, instance slots per row (1..64)
   *    i4 = H  i5 = W of the frame  i7 = R
   *    p0 mode 5's records   p1 its rows   p2 its vertices   p7 the cells (their origins are read)
   *    p4 masks u32[i1, I, R, (R + 31) / 32], TILE-LOCAL: bit b of word w of pixel row y is tile pixel x = 32 w + b
   *    p5 counts i32[i1, I, R]: set bits per pixel row
   *    Pixel (x, y) of slot s is set when x < R, the frame pixel (origin x + x, origin y + y) lies in [0, W) x [0, H), the instance
   *    with ordinal s is kept, and the pixel's centre lies inside at least one of its polygons with nv >= 3, even-odd per polygon.
   *    In tile-local doubled coordinates and 64-bit integers, centre P = (2x + 1, 2y + 1) and vertices 2 v: edge a -> b (the last
   *    vertex to the first included) counts when (ay > Py) != (by > Py) and (Px - ax)(by - ay) < (Py - ay)(bx - ax) for by > ay, >
   *    otherwise; inside = an odd count.  Slots without an instance, instances that are not kept and bits x >= R are zero; every
   *    word and count is written, nothing is accumulated.  An instance's vertices (at most 1024) are staged in LDS.
   *    p0 .. p2 must be what mode 5 wrote for the same i1, T, R and cells: the records of an instance consecutive, its vertices
   *    consecutive and inside the tile.  With other contents no access leaves the extents, but the masks are unspecified.
   * i0 = 2 and i0 = 4 stay refused: the argument tests of modes 1 and 3 launch them with those modes' slots and expect OMNI_E_ARG.
   * OMNI_E_ARG (nothing launched, nothing written): any value outside its range, M != (T - 1) / 9 (mode 3: (T - 1) / 4; mode 5: P !=
   * T / 2 or V != (T - 1) / 2), a grammar outside 0..1, any other i0, a NULL pointer other than p2 of modes 1, 3 and 5, a misaligned
   * pointer.  The pointer check covers exactly these extents.  The op's dtype matters to mode 0 only.  Plan bundles and the
   * model-level entry points do not use it. */
  OMNI_OP_REGION_OCR = OMNI_OP_VISUAL_MATCH + 1,   /* 29 (spelled like the three kinds above) */
  OMNI_OP__END
};

/* token classes of OMNI_OP_REGION_OCR's class table (p1) above the location bins 0..999 */
#define OMNI_OCR_CLASS_STRIP 1000
#define OMNI_OCR_CLASS_TEXT 1001
#define OMNI_OCR_CLASS_HARD 1002
/* mode 5 alone (modes 1 and 3 clamp them to HARD): <sep>, <poly>, </poly> */
#define OMNI_OCR_CLASS_SEP 1003
#define OMNI_OCR_CLASS_POLY 1004
#define OMNI_OCR_CLASS_POLY_END 1005

/* header of the trie block of OMNI_OP_GREEDY_VOCAB_STEP (p7); first / edge_tok / edge_dst follow it, see the op */
#define OMNI_VOCAB_HEADER_BYTES 32
#define OMNI_VOCAB_MAX_NODES 65536     /* nodes of a vocabulary's trie, the root included */
#define OMNI_VOCAB_MAX_LABEL 64        /* tokens of a label */
typedef struct omni_vocab_trie {
  int32_t n_nodes;         /* nodes, the root (node 0) included */
  int32_t n_edges;         /* edges = n_nodes - 1 */
  int32_t longest;         /* tokens of the longest label */
  int32_t reserved[5];
} omni_vocab_trie_t;

/* header of the control block of OMNI_OP_GREEDY_CTRL_STEP (p7); the variable parts follow it, see the op */
#define OMNI_GEN_CTRL_HEADER_BYTES 32
#define OMNI_GEN_CTRL_MAX_BAD 64       /* multi-token bad-word sequences */
#define OMNI_GEN_CTRL_MAX_BAD_LEN 8    /* tokens per sequence */
typedef struct omni_gen_ctrl {
  float penalty;           /* repetition penalty, > 0; 1.0 = none */
  int32_t ngram;           /* no_repeat_ngram_size; -1 = the op's i5, 0 = off */
  int32_t min_new_tokens;  /* eos is -inf while fewer tokens than this have been generated */
  int32_t begin_index;     /* history length (start token included) at which the begin-suppress bitmap applies */
  int32_t n_bad;           /* rows of the bad-word table */
  int32_t bad_stride;      /* 4-byte words per row of the bad-word table */
  int32_t reserved[2];
} omni_gen_ctrl_t;

/* candidate record shared by DETECT_DECODE and NMS (32 bytes) */
typedef struct omni_cand {
  float x1, y1, x2, y2;   /* un-letterboxed, unclamped image pixels */
  float score;
  int32_t cls;            /* arg-max class id */
  int32_t anchor;         /* flat anchor index over strides 8,16,32 (tie-break key) */
  int32_t pad;
} omni_cand_t;
/* NMS scratch `p2` must hold (cap + 1) records: the spare record carries
 * {max coordinate, coordinate-trick flag} of torchvision.ops.batched_nms. */

/* Launch ONE op on `stream` (unit tests, eager mode).
 * Pointer check (here and in omni_plan_create, wherever a device is present; OMNI_CHECK_PTRS=0 turns it off): every non-NULL p[k]
 * must lie in a device allocation known to the HIP runtime, and the byte range the op touches from it (computed for the conv /
 * GEMM family, pools / resizes incl. the extra CBFuse sources, LayerNorm, depthwise conv, split-convert, the fused FFN, detect-decode
 * and NMS; the FIRST BYTE only for the attention, decode-step, crop, hand-off and PNG kinds) must end inside that allocation —
 * otherwise OMNI_E_ARG with the op index, slot and address in omni_last_error() instead of a GPU memory-access fault (which would
 * abort the process).  What it cannot see: an overrun that stays inside one allocation (with a caching allocator: one segment). */
int omni_op_launch(const omni_op_t* op, void* stream);

/* Plan: an immutable list of ops replayed per inference; optionally captured
 * into a hipGraph (one graph launch per screenshot instead of ~300 kernel launches). */
typedef struct omni_plan omni_plan_t;
int omni_plan_create(const omni_op_t* ops, int n_ops, omni_plan_t** out);
int omni_plan_run(omni_plan_t* plan, void* stream);            /* eager replay */
int omni_plan_capture(omni_plan_t* plan, void* stream);        /* build hipGraphExec */
int omni_plan_replay(omni_plan_t* plan, void* stream);         /* launch captured graph */
int omni_plan_num_ops(const omni_plan_t* plan);
void omni_plan_destroy(omni_plan_t* plan);

/* Pillow `precompute_coeffs` + 8bpc fixed-point normalisation, on the host.
 * filter: 0 = LANCZOS (support 3), 1 = BICUBIC (support 2).
 * Writes h_bounds[2*out_size] (xmin, count) and h_coef[out_size*ksize] (22-bit fixed point).
 * Returns ksize (>0) — call with h_bounds == NULL to query ksize only. */
int omni_resample_coeffs(int in_size, int out_size, int filter, int32_t* h_bounds, int32_t* h_coef);

/* HIP-event timing helper so hosts without torch can time a stream region.
 * Records start, runs `plan` `iters` times (graph replay if captured), records
 * stop, synchronises and returns mean milliseconds per iteration in *ms. */
int omni_plan_time(omni_plan_t* plan, void* stream, int iters, float* ms);

/* One EAGER replay with a HIP event around every op (on `stream`): h_ms[i] = device milliseconds of op i in its real
 * sequence.  bench.py derives `roofline.achieved` and the per-kernel-family split of a step from it; the numbers are
 * directly comparable with `rocprofv3 --kernel-trace --stats` of the same replay.  h_ms holds omni_plan_num_ops floats. */
int omni_plan_profile(omni_plan_t* plan, void* stream, float* h_ms);

/* Host mirror of the GEMM kernels' block -> output-tile permutation (XCD-aware order with an optional N partition
 * over XCD groups; csrc/conv_igemm.hip::tile_of_block).  Test/diagnostic entry point, no device work: for block
 * `bid` of a grid over mtiles x ntiles tiles writes the tile (or -1/-1 for a padding block), the grid size and the
 * N-partition count used.  weight_bytes >= 0: choose the partition like the launcher (L2-residency rule);
 * weight_bytes < 0: use `xcd_n` (1, 2, 4 or 8, must divide ntiles). */
int omni_debug_tile_map(int mtiles, int ntiles, int xcd_n, long long weight_bytes, int bid, int* mt, int* nt, int* grid,
                        int* xcd_n_used);

/* What omni_op_launch would launch for an OMNI_OP_CONV op with i20 = 0 or 1, computed by the function the launcher itself calls.
 * Test/diagnostic entry point, no device work, no pointer of the op is dereferenced (p0, p1, p4 must be non-NULL; p5 / p6 count
 * as "workspace / counters present").  The op's own argument errors are returned as they would be by the launch.
 *   out[0] kernel family: 0 = register-staged f32 MFMA, 1 = register-staged f16 MFMA, 2 = split-f16 (i20 = 1)
 *   out[1] BM  out[2] BN  (output tile)   out[3] RB (bytes of K per slice row)
 *   out[4] loader: 0 = generic (ragged K vectors), 1 = aligned, 2 = pointwise, 3 = row-patch (i25)
 *   out[5] split-K count   out[6] 0 = no split-K, 1 = reduce launch, 2 = in-launch combine (i24)   out[7] waves per workgroup */
int omni_debug_conv_cfg(const omni_op_t* op, int out[8]);

/* The launch geometry of an OMNI_OP_VISUAL_MATCH op of mode 1 or 2, computed by the function the launcher itself calls; no device
 * work, no pointer of the op is looked at, i6 is not checked.  The op's own argument errors are returned as the launch returns them.
 *   out[0] groups of 8 queries   out[1] gallery rows per split   out[2] splits   out[3] bytes of the partials buffer (p5) */
int omni_visual_match_cfg(const omni_op_t* op, long long out[4]);

/* ------------------------------------------------------------------------ *
 * Model-level entry points: the two models of the hot path for hosts
 * without Python.  A model is a PLAN BUNDLE file written by omniparser_amd/bundle.py
 * (export_detector / export_captioner): the op lists above over a fixed set of device
 * buffers, with constants and named I/O tensors.  omni_model_load allocates the
 * buffers, uploads the constants, relocates the ops and captures every plan as a
 * hipGraph on a stream owned by the model.  All calls below are SYNCHRONOUS.
 * ------------------------------------------------------------------------ */
typedef struct omni_model omni_model_t;

int  omni_model_load(const char* bundle_path, omni_model_t** out);
void omni_model_destroy(omni_model_t* model);
/* scalars / named device tensors of a bundle ("batch", "img_w", "capacity", "T", ... ; "img", "out_boxes", "x_in", "ids", ...). */
int  omni_model_int(const omni_model_t* model, const char* name, long long* value);
int  omni_model_tensor(const omni_model_t* model, const char* name, void** d_ptr, long long* nbytes);
/* replay one plan of the bundle ("detect", "encode", "step") and wait for it. */
int  omni_model_run(omni_model_t* model, const char* plan_name);

/* Detector = YOLOv9Detector.predict on one batch (ref:util/yolov9.py:115-136: letterbox, network, decode, threshold,
 * batched_nms[:max_det], clamp).  The bundle fixes image size, network size, thresholds, max_det and batch.
 *  images_rgb  n_images x [img_h, img_w, 3] uint8, host (on_device = 0) or device memory
 *  h_boxes     [n_images, max_det, 4] f32 xyxy pixels; h_scores / h_classes [n_images, max_det] (may be NULL);
 *  h_counts    [n_images] number of valid rows per image. */
int  omni_detector_create(const char* bundle_path, omni_model_t** out);
int  omni_detector_infer(omni_model_t* det, const uint8_t* images_rgb, int n_images, int on_device, float* h_boxes, float* h_scores,
                         int32_t* h_classes, int32_t* h_counts);

/* Captioner = the icon_caption loop of ref:util/utils.py:88-132 on one screenshot: crop each box, cv2.resize 64x64, processor
 * (bicubic to R x R on the 768 path, rescale, normalise), Florence-2 generate(num_beams=1, max_new_tokens) — greedy ids.
 *  image_rgb   [img_h, img_w, 3] uint8, host or device;   h_boxes_px [n, 4] int32 xyxy pixels (any n: micro-batches of the
 *  bundle's capacity);   h_ids [n, T] int32, T = omni_model_int("T") = max_new_tokens + 1; rows are padded with the pad id
 *  after EOS exactly as generate() pads them. */
int  omni_captioner_create(const char* bundle_path, omni_model_t** out);
int  omni_captioner_caption(omni_model_t* cap, const uint8_t* image_rgb, int on_device, int img_h, int img_w, const int32_t* h_boxes_px,
                            int n, int32_t* h_ids);

#ifdef __cplusplus
}
#endif
#endif /* OMNI_AMD_H */
