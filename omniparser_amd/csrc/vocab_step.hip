// OMNI_OP_GREEDY_VOCAB_STEP: greedy decoding step over a CLOSED VOCABULARY — the caption is always exactly one label of a set the
// caller gave.  transformers' PrefixConstrainedLogitsProcessor takes a Python callable per step; a captured step graph cannot call
// one, so the set is compiled to a trie (CSR, include/omni_amd.h: struct omni_vocab_trie) that lies in device memory and is read at
// every step: one plan and one graph serve every vocabulary, as the control block of OMNI_OP_GREEDY_CTRL_STEP does for its settings.
//
//   greedy_vocab_step   final_logits_bias + NoRepeatNGram + PrefixConstrained (the children of the row's trie node) + ForcedBOS/EOS
//                       + argmax + EOS/pad bookkeeping + the row's next node
//                       hf:generation/utils.py _get_logits_processor, hf:generation/logits_process.py (NoRepeatNGram,
//                       PrefixConstrained, ForcedBOSToken, ForcedEOSToken)
//
// A row reads its logits ONLY at the edge tokens of its node — a handful of scattered loads instead of the two passes over 51289
// entries of the other greedy kernels.  The helpers below are copies of the few lines of caption_ops.hip (whose kernels keep their
// machine code: nothing there is touched).
#include "omni_internal.h"

#pragma clang fp contract(off)

namespace {

template <typename T> __device__ __forceinline__ float ldf(const T* p) { return ElemTraits<T>::to_f32(*p); }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

struct VocabArgs {
  const void* logits; const float* bias; int* ids; int* finished; const int* step;
  int B, V, ldl, T, max_new, ngram, bos, eos, pad, forced_bos, forced_eos;
  float* logp;                         // SCORES instantiation only: f32 [B, T] log-probability of every emitted token
  int* node;                           // i32 [B]: the row's trie node, 0 = root, -1 = left the trie; read and written
  const int* trie; int trie_bytes;     // the trie block and its size (i12): nothing beyond it is read
};

// One workgroup per row.  The n-gram ban is exact for any history: all 256 threads compare their n-gram start positions with the
// current prefix and append the followers of the matching ones to a list of capacity T in LDS (as greedy_step_long_kernel does);
// an edge is banned when its token is in the list.  The list is short (one entry per earlier occurrence of the prefix) and a node
// has few edges everywhere but at the root, where the history is one or two tokens long.
// Header values are clamped to what trie_bytes can hold and edge ranges to the edge arrays, so a block that lies about itself is
// read wrongly but never out of bounds; edge tokens outside 0..V-1 are skipped.  Edge tokens ascend within a node (the host sorts
// them), so "first maximum in this thread's stride, then the lower token among equals" is the lowest token id among equals.
template <typename T, bool SCORES>
__global__ __launch_bounds__(256) void greedy_vocab_step_kernel(VocabArgs a) {
  OMNI_DYN_LDS(int, follow);           // [T] followers of the n-grams that match the current prefix
  __shared__ float sval[256];
  __shared__ int sidx[256];
  __shared__ int nmatch;
  __shared__ int snext;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int st = *a.step;              // tokens so far = st + 1 (ids[b][0..st]); we write ids[b][st+1]
  if (st < 0 || st + 1 >= a.T) return; // a step outside the plan's positions writes nothing (uniform over the grid)
  int* ids = a.ids + b * a.T;
  const int cur_len = st + 1;
  // ---- the trie block, clamped to trie_bytes
  const int words = a.trie_bytes >> 2;
  int n_nodes = 0, n_edges = 0;
  if (words >= OMNI_VOCAB_HEADER_BYTES / 4 + 1) {
    n_nodes = max(0, min(min(a.trie[0], OMNI_VOCAB_MAX_NODES), words - OMNI_VOCAB_HEADER_BYTES / 4 - 1));
    n_edges = max(0, min(a.trie[1], (words - OMNI_VOCAB_HEADER_BYTES / 4 - 1 - n_nodes) >> 1));
  }
  const int* first = a.trie + OMNI_VOCAB_HEADER_BYTES / 4;      // [n_nodes + 1]
  const int* edge_tok = first + n_nodes + 1;                    // [n_edges]
  const int* edge_dst = edge_tok + n_edges;                     // [n_edges]
  const int nd = a.node[b];
  int e0 = 0, e1 = 0;
  if (nd >= 0 && nd < n_nodes) {
    e0 = max(0, min(first[nd], n_edges));
    e1 = max(e0, min(first[nd + 1], n_edges));
  }
  if (tid == 0) { nmatch = 0; snext = -1; }
  __syncthreads();
  // NoRepeatNGram: ban tokens completing an n-gram already generated (incl. decoder start token)
  const int n = a.ngram;
  const int nstart = n > 0 && cur_len + 1 >= n ? min(cur_len - n + 1, a.T) : 0;     // start positions i with i + n - 1 < cur_len
  for (int i = tid; i < nstart; i += 256) {
    bool match = true;
    for (int j = 0; j < n - 1; ++j)
      if (ids[i + j] != ids[cur_len - (n - 1) + j]) { match = false; break; }
    if (match) follow[atomicAdd(&nmatch, 1)] = ids[i + n - 1];
  }
  __syncthreads();
  const int nm = nmatch;
  int forced = -1;
  if (a.forced_bos >= 0 && cur_len == 1) forced = a.forced_bos;
  if (a.forced_eos >= 0 && cur_len == a.max_new) forced = a.forced_eos;   // max_length - 1 == max_new (start token + max_new)
  int tok;
  [[maybe_unused]] float lp = 0.0f;
  if (forced >= 0) {
    tok = forced;
  } else {
    const T* lg = (const T*)a.logits + (long long)b * a.ldl;
    // the processed score of edge e: -inf for a token outside the vocabulary or a banned one
    auto proc = [&](int e) {
      const int t = edge_tok[e];
      if (t < 0 || t >= a.V) return -INFINITY;
      float x = ldf(lg + t) + (a.bias ? a.bias[t] : 0.0f);
      for (int q = 0; q < nm; ++q) if (follow[q] == t) x = -INFINITY;
      return x;
    };
    float best = -INFINITY; int bi = 0x7fffffff;
    for (int e = e0 + tid; e < e1; e += 256) {
      const float x = proc(e);
      if (x > best) { best = x; bi = edge_tok[e]; }      // first max within this thread's ascending stride
    }
    sval[tid] = best; sidx[tid] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) {
        float ov = sval[tid + s]; int oi = sidx[tid + s];
        if (ov > sval[tid] || (ov == sval[tid] && oi < sidx[tid])) {
          sval[tid] = ov; sidx[tid] = oi;
        }
      }
      __syncthreads();
    }
    tok = sidx[0];
    // no edge compared greater than -inf (node -1, a leaf, every child banned, NaN / -inf logits): position 0, as the other greedy
    // kernels and torch.argmax; never hand an out-of-range id to the next step's embedding gather
    if (tok < 0 || tok >= a.V) tok = 0;
    if constexpr (SCORES) {
      const float mx = sval[0];                 // the processed maximum (-inf for a degenerate row: lp is then unspecified)
      __syncthreads();                          // every thread holds mx and tok before sval is reused
      float sum = 0.f;
      for (int e = e0 + tid; e < e1; e += 256) sum += expf(proc(e) - mx);
      sum = wave_sum(sum);
      if ((tid & 63) == 0) sval[tid >> 6] = sum;
      __syncthreads();
      lp = 0.0f - logf(((sval[0] + sval[1]) + sval[2]) + sval[3]);   // +0.0 at a node with one allowed child
    }
  }
  // the child the emitted token leads to (the forced token moves the node too); at most one edge of a node carries a token
  for (int e = e0 + tid; e < e1; e += 256)
    if (edge_tok[e] == tok) snext = edge_dst[e];
  __syncthreads();
  if (tid == 0) {
    int fin = a.finished[b];
    if (fin) tok = a.pad;                       // finished rows keep emitting pad (hf utils.py:2925-2929)
    ids[st + 1] = tok;
    if constexpr (SCORES) a.logp[(long long)b * a.T + st + 1] = fin ? 0.0f : lp;
    if (!fin && tok == a.eos) a.finished[b] = 1;
    if (!fin) a.node[b] = snext;                // finished rows leave their node alone
  }
}

__global__ void vocab_step_inc_kernel(int* step) { if (threadIdx.x == 0 && blockIdx.x == 0) *step += 1; }

}  // namespace

int omni_launch_vocab_step(const omni_op_t* op, hipStream_t s) {
  VocabArgs a{};
  a.logits = op->p[0]; a.bias = (const float*)op->p[1]; a.ids = (int*)op->p[2]; a.finished = (int*)op->p[3];
  a.logp = (float*)op->p[4]; a.node = (int*)op->p[5]; a.step = (const int*)op->p[6]; a.trie = (const int*)op->p[7];
  a.B = op->i[0]; a.V = op->i[1]; a.ldl = op->i[2]; a.T = op->i[3]; a.max_new = op->i[4]; a.ngram = op->i[5];
  a.bos = op->i[6]; a.eos = op->i[7]; a.pad = op->i[8]; a.forced_bos = op->i[9]; a.forced_eos = op->i[10];
  a.trie_bytes = op->i[12];
  OMNI_REQUIRE(a.logits && a.ids && a.finished && a.step && a.B > 0 && a.V > 0 && a.ldl >= a.V && a.T >= a.max_new + 1 && a.max_new >= 1,
               "greedy_vocab_step: bad arguments");
  OMNI_REQUIRE((unsigned long long)a.logits % (op->dtype == OMNI_F32 ? 4 : 2) == 0, "greedy_vocab_step: logits not aligned to their element");
  OMNI_REQUIRE(a.node, "greedy_vocab_step: p5 (the rows' trie nodes, i32[B]) is NULL");
  OMNI_REQUIRE(a.trie && (unsigned long long)a.trie % 4 == 0, "greedy_vocab_step: p7 (trie block) is NULL or not 4-byte aligned");
  OMNI_REQUIRE(a.trie_bytes >= OMNI_VOCAB_HEADER_BYTES + 4, "greedy_vocab_step: a trie block of %d bytes (i12) cannot hold the header and one "
               "node (%d bytes)", a.trie_bytes, OMNI_VOCAB_HEADER_BYTES + 4);
  const size_t lds = (size_t)a.T * 4;
  OMNI_REQUIRE(lds <= 48 * 1024, "greedy_vocab_step: %d positions exceed the n-gram LDS", a.T);
  const bool sc = a.logp != nullptr;
  if (op->dtype == OMNI_F32) {
    if (sc) hipLaunchKernelGGL((greedy_vocab_step_kernel<float, true>), dim3(a.B), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((greedy_vocab_step_kernel<float, false>), dim3(a.B), dim3(256), lds, s, a);
  } else if (op->dtype == OMNI_F16) {
    if (sc) hipLaunchKernelGGL((greedy_vocab_step_kernel<half_t, true>), dim3(a.B), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((greedy_vocab_step_kernel<half_t, false>), dim3(a.B), dim3(256), lds, s, a);
  } else {
    omni_set_error("greedy_vocab_step: unsupported dtype %d", op->dtype);
    return OMNI_E_ARG;
  }
  if (op->i[11]) hipLaunchKernelGGL(vocab_step_inc_kernel, dim3(1), dim3(64), 0, s, (int*)op->p[6]);   // i11: advance the step counter
  OMNI_HIP_CHECK(hipGetLastError());
  return OMNI_OK;
}
