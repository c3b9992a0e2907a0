// Device-resident beam search of generate (mrblip/search.py beam_search restated on device state): candidate selection over the
// vocabulary, the beam / hypothesis-pool bookkeeping, the final ranking and the re-ordering of the self-attention K / V cache.
// Nothing here uses a float atomic, nothing waits for the host, and every reduction runs in a fixed order: two runs give the same bits.
//
// ORDER of candidates everywhere: higher score first, equal scores by LOWER flat index (beam * V + token); pool entries: higher score
// first, equal scores by lower pool slot.  (At step 0 the beams 1..K-1 carry -1e9 and all their candidates tie exactly.)
//
// Second half of the file: the device-resident sampler (mrblip/search.py sample_search — nucleus sampling and greedy decoding on warped raw
// logits), which shares the per-chunk selection with the beam search.
#include "common.h"
#include "../../include/mrblip_hip.h"
#include <limits.h>
#include <math.h>

#define BS_CHUNK 2048      // vocabulary entries per selection workgroup: 256 lanes x 8
#define BS_MAX_SPLIT 64    // => V <= 131072
#define BS_MAX_K 16

namespace {

struct Key {
  float s;
  int i;
};
// "nothing": loses against every real candidate (a real -inf score still has a real index)
__device__ __forceinline__ Key key_none() { return {-INFINITY, INT_MAX}; }
__device__ __forceinline__ bool key_before(const Key a, const Key b) { return a.s > b.s || (a.s == b.s && a.i < b.i); }
// the better of a and b among the keys that come strictly AFTER `last` in the order (selection without marking anything as taken)
__device__ __forceinline__ Key key_pick(const Key best, const Key x, const Key last) {
  return (key_before(last, x) && key_before(x, best)) ? x : best;
}
__device__ __forceinline__ Key wave_best(Key k) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Key other;
    other.s = __shfl_xor(k.s, o, 64);
    other.i = __shfl_xor(k.i, o, 64);
    if (key_before(other, k)) k = other;
  }
  return k;
}
// best key of a 256-lane workgroup, returned to every lane; slot[4] is LDS the caller alternates between calls (one barrier per call)
__device__ __forceinline__ Key block_best(Key k, Key* slot) {
  k = wave_best(k);
  if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = k;
  __syncthreads();
  Key b = slot[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (key_before(slot[w], b)) b = slot[w];
  return b;
}

// LDS bitmap of the chunk [base, base + BS_CHUNK): bit set for every token id among the row's first cur_len sequence tokens (the
// repetition penalty's set; left empty when pen == 1).  256 lanes; the bitmap is complete when the call returns.
__device__ __forceinline__ void chunk_mark_seen(uint32_t* seen, const int* __restrict__ seq_row, int cur_len, int base, float pen) {
  const int tid = threadIdx.x;
  if (tid < BS_CHUNK / 32) seen[tid] = 0u;
  __syncthreads();
  if (pen != 1.0f) {
    for (int j = tid; j < cur_len; j += 256) {
      const int t = seq_row[j] - base;
      if (t >= 0 && t < BS_CHUNK) atomicOr(&seen[t >> 5], 1u << (t & 31));   // (integer OR: order free)
    }
  }
  __syncthreads();
}
__device__ __forceinline__ bool chunk_seen(const uint32_t* seen, int c) { return (seen[c >> 5] >> (c & 31)) & 1u; }
// the n best of the workgroup's 256 x 8 keys, best first, to os / oi (key_none once the chunk is exhausted): n selections without marking
__device__ __forceinline__ void chunk_select(const Key (&mine)[8], int n, Key (*slots)[4], float* __restrict__ os, int* __restrict__ oi) {
  Key last = {INFINITY, -1};
  for (int it = 0; it < n; ++it) {
    Key b = key_none();
#pragma unroll
    for (int j = 0; j < 8; ++j) b = key_pick(b, mine[j], last);
    b = block_best(b, slots[it & 1]);
    if (threadIdx.x == 0) {
      os[it] = b.s;
      oi[it] = b.i;
    }
    last = b;
  }
}

// ---- pass 1: per (row, vocabulary chunk) the maximum and the sum of exp(x - max)
__global__ __launch_bounds__(256) void beam_lse_kernel(const float* __restrict__ logits, long long ldl, int V, int NS, float* __restrict__ pm,
                                                        float* __restrict__ ps) {
  const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
  const float* x = logits + (long long)row * ldl;
  float v[8];
  float m = -INFINITY;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = sp * BS_CHUNK + j * 256 + tid;
    v[j] = c < V ? x[c] : -INFINITY;
    m = fmaxf(m, v[j]);
  }
  __shared__ float red[4];
  m = wave_max(m);
  if ((tid & 63) == 0) red[tid >> 6] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  float s = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int j = 0; j < 8; ++j) s += expf(v[j] - m);
  }
  s = wave_sum(s);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    pm[row * NS + sp] = m;
    ps[row * NS + sp] = (red[0] + red[1]) + (red[2] + red[3]);
  }
}

// ---- pass 2: per (row, chunk) the 2K best candidate scores of the chunk, best first
// score = log_softmax(logits)[row, v] (repetition penalty on tokens of the row's sequence, EOS -> -inf while masked) + beam_score[row]
__global__ __launch_bounds__(256) void beam_select_kernel(const float* __restrict__ logits, long long ldl, const float* __restrict__ beam_scores,
                                                           const int* __restrict__ seqs, long long lds_, const float* __restrict__ pm,
                                                           const float* __restrict__ ps, int NS, int K, int V, int cur_len, int eos_masked, int eos_id,
                                                           float pen, float* __restrict__ part_s, int* __restrict__ part_i) {
  const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
  const int base = sp * BS_CHUNK;
  __shared__ uint32_t seen[BS_CHUNK / 32];
  __shared__ Key slots[2][4];
  chunk_mark_seen(seen, seqs + (long long)row * lds_, cur_len, base, pen);
  // log-sum-exp of the row from the chunk partials, in chunk order
  float M = -INFINITY;
  for (int s = 0; s < NS; ++s) M = fmaxf(M, pm[row * NS + s]);
  float S = 0.f;
  for (int s = 0; s < NS; ++s) {
    const float m = pm[row * NS + s];
    if (m > -INFINITY) S += ps[row * NS + s] * expf(m - M);
  }
  const float lse = M + logf(S);
  const float bs = beam_scores[row];
  const int beam = row % K;
  const float* x = logits + (long long)row * ldl;
  Key mine[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = j * 256 + tid, v = base + c;
    mine[j] = key_none();
    if (v < V) {
      float lp = x[v] - lse;
      if (chunk_seen(seen, c)) lp = lp < 0.f ? lp * pen : lp / pen;
      if (eos_masked && v == eos_id) lp = -INFINITY;
      mine[j].s = lp + bs;
      mine[j].i = beam * V + v;
    }
  }
  chunk_select(mine, 2 * K, slots, part_s + ((long long)row * NS + sp) * 2 * K, part_i + ((long long)row * NS + sp) * 2 * K);
}

// ---- pass 3: per clip, merge the K * NS sorted lists into the clip's 2K best (a lane owns up to four lists and offers their heads)
__global__ __launch_bounds__(256) void beam_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_i, int NS, int K,
                                                          float* __restrict__ cand_s, int* __restrict__ cand_i) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int nl = K * NS, n2 = 2 * K;
  const float* ls = part_s + (long long)b * nl * n2;
  const int* li = part_i + (long long)b * nl * n2;
  __shared__ Key slots[2][4];
  int ptr[4] = {0, 0, 0, 0};
  for (int it = 0; it < n2; ++it) {
    Key head[4];
    Key best = key_none();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int l = tid + j * 256;
      head[j] = key_none();
      if (l < nl && ptr[j] < n2) {
        head[j].s = ls[l * n2 + ptr[j]];
        head[j].i = li[l * n2 + ptr[j]];
      }
      if (key_before(head[j], best)) best = head[j];
    }
    best = block_best(best, slots[it & 1]);
    if (tid == 0) {
      cand_s[b * n2 + it] = best.s;
      cand_i[b * n2 + it] = best.i;
    }
    if (best.i != INT_MAX) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (head[j].i == best.i) ptr[j]++;    // (flat indices are unique)
    }
  }
}

// slot of the pool's worst entry: lowest score, equal scores -> lowest slot (Python's min() over the pool list)
__device__ __forceinline__ int pool_worst(const float* sc, int n) {
  int w = 0;
  for (int j = 1; j < n; ++j)
    if (sc[j] < sc[w]) w = j;
  return w;
}
// search.py pool_add: returns the slot the hypothesis goes to, or -1
__device__ __forceinline__ int pool_place(float* sc, int& n, int K, float score) {
  int slot;
  if (n < K) slot = n++;
  else {
    slot = pool_worst(sc, n);
    if (!(score > sc[slot])) return -1;
  }
  sc[slot] = score;
  return slot;
}

struct AdvanceArgs {
  const float* cand_s;
  const int* cand_i;
  const int* seq_in;
  int* seq_out;
  long long lds;
  float* beam_scores;
  int *parents, *tokens;
  float* pool_score;
  int *pool_len, *pool_seq, *pool_n, *done, *done_count;
  int K, V, cur_len, eos_id, pad_id;
  float len_pow;
};

// ---- search.py:134-160 for one clip
__global__ __launch_bounds__(64) void beam_advance_kernel(const AdvanceArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x, K = a.K, L = a.cur_len;
  const int* sin = a.seq_in + (long long)b * K * a.lds;
  int* sout = a.seq_out + (long long)b * K * a.lds;
  if (a.done[b]) {   // padded beams with score 0 and identity parents, like HF
    for (int k = 0; k < K; ++k) {
      for (int j = tid; j < L; j += 64) sout[k * a.lds + j] = sin[k * a.lds + j];
      if (tid == 0) sout[k * a.lds + L] = a.pad_id;
    }
    if (tid < K) {
      a.beam_scores[b * K + tid] = 0.f;
      a.parents[b * K + tid] = b * K + tid;
      a.tokens[b * K + tid] = a.pad_id;
    }
    return;
  }
  __shared__ int s_par[BS_MAX_K], s_tok[BS_MAX_K], ins_slot[BS_MAX_K], ins_beam[BS_MAX_K], s_nins;
  __shared__ float s_sc[BS_MAX_K], s_pool[BS_MAX_K];
  if (tid == 0) {
    int n = a.pool_n[b], kept = 0, nins = 0;
    for (int j = 0; j < n; ++j) s_pool[j] = a.pool_score[b * K + j];
    for (int rank = 0; rank < 2 * K && kept < K; ++rank) {
      const float sc = a.cand_s[b * 2 * K + rank];
      const int ix = a.cand_i[b * 2 * K + rank];
      if (ix < 0 || ix >= K * a.V) continue;
      const int beam = ix / a.V, tok = ix - beam * a.V;
      if (tok == a.eos_id) {
        if (rank >= K) continue;
        const int slot = pool_place(s_pool, n, K, sc / a.len_pow);   // generated length = cur_len (the EOS counts, the start token does not)
        if (slot >= 0) {
          ins_slot[nins] = slot;
          ins_beam[nins++] = beam;
        }
        continue;
      }
      s_par[kept] = beam;
      s_tok[kept] = tok;
      s_sc[kept++] = sc;
    }
    for (; kept < K; ++kept) {   // cannot happen (at most K of the 2K best are EOS): keep the state well formed anyway
      s_par[kept] = kept;
      s_tok[kept] = a.pad_id;
      s_sc[kept] = -1e9f;
    }
    for (int j = 0; j < n; ++j) a.pool_score[b * K + j] = s_pool[j];
    a.pool_n[b] = n;
    s_nins = nins;
    if (n >= K) {   // early_stopping=False: can any running beam still beat the pool's worst?
      const float worst = s_pool[pool_worst(s_pool, n)];
      if (worst >= a.cand_s[b * 2 * K] / a.len_pow) {
        a.done[b] = 1;
        atomicAdd(a.done_count, 1);   // (integer count: order free)
      }
    }
  }
  __syncthreads();
  for (int e = 0; e < s_nins; ++e) {   // in candidate order: a later entry may reuse a slot
    int* dst = a.pool_seq + ((long long)b * K + ins_slot[e]) * a.lds;
    const int* src = sin + ins_beam[e] * a.lds;
    for (int j = tid; j < L; j += 64) dst[j] = src[j];
    if (tid == 0) {
      dst[L] = a.eos_id;
      a.pool_len[b * K + ins_slot[e]] = L + 1;
    }
    __syncthreads();
  }
  for (int k = 0; k < K; ++k) {
    const int* src = sin + s_par[k] * a.lds;
    for (int j = tid; j < L; j += 64) sout[k * a.lds + j] = src[j];
    if (tid == 0) sout[k * a.lds + L] = s_tok[k];
  }
  if (tid < K) {
    a.beam_scores[b * K + tid] = s_sc[tid];
    a.parents[b * K + tid] = b * K + s_par[tid];
    a.tokens[b * K + tid] = s_tok[tid];
  }
}

// ---- search.py:164-170: running beams of unfinished clips join the pool; the num_return best leave as [length, score bits, tokens...]
__global__ __launch_bounds__(64) void beam_finalize_kernel(const int* __restrict__ seq, long long lds_, const float* __restrict__ beam_scores,
                                                            float* pool_score, int* pool_len, int* pool_seq, int* pool_n, const int* __restrict__ done,
                                                            int K, int cur_len, float len_pow, int num_return, int* __restrict__ out) {
  const int b = blockIdx.x, tid = threadIdx.x;
  __shared__ float s_pool[BS_MAX_K];
  __shared__ int s_slot, s_n, s_rank[BS_MAX_K];
  if (tid == 0) {
    s_n = pool_n[b];
    for (int j = 0; j < s_n; ++j) s_pool[j] = pool_score[b * K + j];
  }
  __syncthreads();
  if (!done[b]) {
    for (int k = 0; k < K; ++k) {
      if (tid == 0) {
        int n = s_n;
        s_slot = pool_place(s_pool, n, K, beam_scores[b * K + k] / len_pow);
        s_n = n;
      }
      __syncthreads();
      if (s_slot >= 0) {
        int* dst = pool_seq + ((long long)b * K + s_slot) * lds_;
        const int* src = seq + ((long long)b * K + k) * lds_;
        for (int j = tid; j < cur_len; j += 64) dst[j] = src[j];
        if (tid == 0) pool_len[b * K + s_slot] = cur_len;
      }
      __syncthreads();
    }
  }
  if (tid == 0) {
    const int n = s_n;
    pool_n[b] = n;
    for (int j = 0; j < n; ++j) pool_score[b * K + j] = s_pool[j];
    uint32_t used = 0u;
    for (int r = 0; r < num_return; ++r) {   // selection in (score descending, slot ascending) order
      int best = -1;
      for (int j = 0; j < n; ++j)
        if (!((used >> j) & 1u) && (best < 0 || s_pool[j] > s_pool[best])) best = j;
      s_rank[r] = best;
      if (best >= 0) used |= 1u << best;
    }
  }
  __syncthreads();
  const long long ldo = lds_ + 2;
  for (int r = 0; r < num_return; ++r) {
    int* o = out + ((long long)b * num_return + r) * ldo;
    const int slot = s_rank[r];
    const int len = slot >= 0 ? pool_len[b * K + slot] : 0;
    if (tid == 0) {
      o[0] = len;
      o[1] = slot >= 0 ? __float_as_int(s_pool[slot]) : 0;
    }
    const int* src = pool_seq + ((long long)b * K + (slot >= 0 ? slot : 0)) * lds_;
    for (int j = tid; j < len; j += 64) o[2 + j] = src[j];
  }
}

// ---- dst[plane, r, :t, :] = src[plane, parents[r], :t, :]: rows of t * inner contiguous bf16, moved 16 bytes per lane
__global__ __launch_bounds__(256) void kv_gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, const int* __restrict__ parents,
                                                              int R, long long row16, long long n16) {
  const int r = blockIdx.x, plane = blockIdx.y;
  int p = parents[r];
  if (p < 0 || p >= R) p = r;   // (never read outside the cache, whatever the index buffer holds)
  const uint4* s = src + ((long long)plane * R + p) * row16;
  uint4* d = dst + ((long long)plane * R + r) * row16;
  for (long long i = (long long)blockIdx.z * 256 + threadIdx.x; i < n16; i += 256ll * gridDim.z) d[i] = s[i];
}

// ================================================================================================ device-resident sampler
// mrblip/search.py sample_search on device state.  Candidates are WARPED RAW LOGITS (no log-softmax pass: a softmax is only ever needed
// over the k <= 64 survivors); order: higher score first, equal scores by lower token id.
#define SS_MAX_K 64
#define SS_MAX_ROWS 256

// ---- pass 1: per (row, chunk) the k best warped logits of the chunk, best first
__global__ __launch_bounds__(256) void sample_select_kernel(const float* __restrict__ logits, long long ldl, const int* __restrict__ seqs,
                                                             long long lds_, int NS, int k, int V, int cur_len, int eos_masked, int eos_id, float pen,
                                                             float* __restrict__ part_s, int* __restrict__ part_i) {
  const int row = blockIdx.y, sp = blockIdx.x, tid = threadIdx.x;
  const int base = sp * BS_CHUNK;
  __shared__ uint32_t seen[BS_CHUNK / 32];
  __shared__ Key slots[2][4];
  chunk_mark_seen(seen, seqs + (long long)row * lds_, cur_len, base, pen);
  const float* x = logits + (long long)row * ldl;
  Key mine[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = j * 256 + tid, v = base + c;
    mine[j] = key_none();
    if (v < V) {
      float s = x[v];
      if (chunk_seen(seen, c)) s = s < 0.f ? s * pen : s / pen;
      if (eos_masked && v == eos_id) s = -INFINITY;
      mine[j].s = s;
      mine[j].i = v;
    }
  }
  chunk_select(mine, k, slots, part_s + ((long long)row * NS + sp) * k, part_i + ((long long)row * NS + sp) * k);
}

// ---- pass 2: per row, merge the NS <= 64 sorted lists (lane l offers the head of list l) into cand[row, 0..k); slots k..63: (-inf, -1)
__global__ __launch_bounds__(64) void sample_merge_kernel(const float* __restrict__ part_s, const int* __restrict__ part_i, int NS, int k,
                                                          float* __restrict__ cand_s, int* __restrict__ cand_i) {
  const int row = blockIdx.x, tid = threadIdx.x;
  const float* ls = part_s + ((long long)row * NS + tid) * k;
  const int* li = part_i + ((long long)row * NS + tid) * k;
  int ptr = 0;
  for (int it = 0; it < k; ++it) {
    Key head = key_none();
    if (tid < NS && ptr < k) {
      head.s = ls[ptr];
      head.i = li[ptr];
    }
    const Key best = wave_best(head);
    if (tid == 0) {
      cand_s[row * SS_MAX_K + it] = best.s;
      cand_i[row * SS_MAX_K + it] = best.i;
    }
    if (best.i != INT_MAX && head.i == best.i) ptr++;   // (token ids are unique within a row)
  }
  if (tid >= k) {
    cand_s[row * SS_MAX_K + tid] = -INFINITY;
    cand_i[row * SS_MAX_K + tid] = -1;
  }
}

struct SampleArgs {
  const float* cand_s;
  const int* cand_i;
  int* seq;
  long long lds;
  int *tokens, *unfinished, *length, *done_count;
  const float* uniforms;
  uint32_t seed;
  int R, V, k, cur_len, eos_id, pad_id, greedy;
  float temperature, top_p;
};

// rank drawn for one row: softmax over the k candidates at the temperature, HF's top-p cut restated for a descending list, one draw.
// fp64 over at most 64 values, every sum sequential in rank order, no contraction: the decisions can be reproduced bit for bit on a host.
__device__ int sample_rank(const float* __restrict__ cs, int k, double T, double top_p, double u) {
#pragma clang fp contract(off)
  const double w0 = (double)cs[0] / T;
  double Z = 0.0;
  for (int i = 0; i < k; ++i) Z += exp((double)cs[i] / T - w0);
  // the kept set is a prefix of n ranks; P = P_{n-1}
  const double thr = (1.0 - top_p) * Z;
  double P = exp(w0 - w0);
  int n = 1;
  for (int i = 1; i < k; ++i) {
    const double p = exp((double)cs[i] / T - w0);
    const bool keep = top_p >= 1.0 ? p > 0.0 : Z - P > thr;   // (P is P_{i-1} here)
    if (!keep) break;
    P += p;
    n = i + 1;
  }
  const double target = u * P;
  double acc = 0.0;
  for (int i = 0; i < n; ++i) {
    acc += exp((double)cs[i] / T - w0);
    if (acc > target) return i;
  }
  return n - 1;
}

// ---- search.py sample_search lines 70-82 for every row: one workgroup, lane r owns row r
__global__ __launch_bounds__(SS_MAX_ROWS) void sample_advance_kernel(const SampleArgs a) {
  const int r = threadIdx.x;
  int finished = 0;
  if (r < a.R) {
    const float* cs = a.cand_s + r * SS_MAX_K;
    int rank = 0;
    if (!a.greedy && a.k > 1) {
      const int t = a.cur_len - 1;
      const double u = a.uniforms ? (double)a.uniforms[(long long)t * a.R + r]
                                  : (double)(mrb_hash((uint32_t)(r * 256 + t), a.seed, MRB_SITE_SAMPLE) >> 8) * (1.0 / 16777216.0);
      rank = sample_rank(cs, a.k, (double)a.temperature, (double)a.top_p, u);
    }
    int tok = a.cand_i[r * SS_MAX_K + rank];
    if (tok < 0 || tok >= a.V) tok = a.pad_id;   // (a row of NaNs ranks nothing: never hand the decoder an index outside its table)
    int unf = a.unfinished[r];
    if (!unf) tok = a.pad_id;
    a.seq[r * a.lds + a.cur_len] = tok;
    a.tokens[r] = tok;
    if (unf && tok == a.eos_id) {
      unf = 0;
      a.unfinished[r] = 0;
      a.length[r] = a.cur_len + 1;
    }
    finished = !unf;
  }
  __shared__ int part[SS_MAX_ROWS / 64];
  const int n = __popcll(__ballot(finished));
  if ((r & 63) == 0) part[r >> 6] = n;
  __syncthreads();
  if (r == 0) a.done_count[0] = (part[0] + part[1]) + (part[2] + part[3]);
}

}  // namespace

extern "C" int mrblip_beam_topk(const float* logits, long long ldl, const float* beam_scores, const int* seqs, long long lds_, int R, int K, int V,
                                int cur_len, int min_length, int eos_id, float repetition_penalty, float* cand_score, int* cand_index, void* ws,
                                long long ws_bytes, hipStream_t stream) {
  MRB_REQUIRE(K >= 1 && K <= BS_MAX_K, "mrblip_beam_topk: K = %d beams, 1..%d supported", K, BS_MAX_K);
  MRB_REQUIRE(V >= 2 * K, "mrblip_beam_topk: V = %d < 2K = %d candidates per clip cannot be ranked", V, 2 * K);
  MRB_REQUIRE(R >= K && R % K == 0, "mrblip_beam_topk: R = %d rows is not a multiple of K = %d", R, K);
  const int NS = (V + BS_CHUNK - 1) / BS_CHUNK;
  MRB_REQUIRE(NS <= BS_MAX_SPLIT, "mrblip_beam_topk: V = %d above %d", V, BS_MAX_SPLIT * BS_CHUNK);
  MRB_REQUIRE(cur_len >= 1 && lds_ >= cur_len && ldl >= V && repetition_penalty > 0.f, "mrblip_beam_topk: bad cur_len / leading dimension / penalty");
  const long long need = 4ll * R * NS * (2 + 4 * K);
  MRB_REQUIRE(logits && beam_scores && seqs && cand_score && cand_index && ws && ws_bytes >= need && ((uintptr_t)ws % 16) == 0,
              "mrblip_beam_topk: null buffer or workspace below %lld bytes (4 * R * ceil(V / 2048) * (2 + 4K))", need);
  float* pm = (float*)ws;
  float* ps = pm + (long long)R * NS;
  float* part_s = ps + (long long)R * NS;
  int* part_i = (int*)(part_s + (long long)R * NS * 2 * K);
  hipLaunchKernelGGL(beam_lse_kernel, dim3(NS, R), dim3(256), 0, stream, logits, ldl, V, NS, pm, ps);
  hipLaunchKernelGGL(beam_select_kernel, dim3(NS, R), dim3(256), 0, stream, logits, ldl, beam_scores, seqs, lds_, pm, ps, NS, K, V, cur_len,
                     cur_len < min_length ? 1 : 0, eos_id, repetition_penalty, part_s, part_i);
  hipLaunchKernelGGL(beam_merge_kernel, dim3(R / K), dim3(256), 0, stream, part_s, part_i, NS, K, cand_score, cand_index);
  return mrblip_check_launch("mrblip_beam_topk");
}

extern "C" int mrblip_beam_advance(const float* cand_score, const int* cand_index, const int* seq_in, int* seq_out, long long lds_,
                                   float* beam_scores, int* parents, int* tokens, float* pool_score, int* pool_len, int* pool_seq, int* pool_n,
                                   int* done, int* done_count, int B, int K, int V, int cur_len, int eos_id, int pad_id, float len_pow,
                                   hipStream_t stream) {
  MRB_REQUIRE(K >= 1 && K <= BS_MAX_K && B >= 1 && V >= 2 * K, "mrblip_beam_advance: B = %d, K = %d (1..%d), V = %d (>= 2K)", B, K, BS_MAX_K, V);
  MRB_REQUIRE(cur_len >= 1 && lds_ >= cur_len + 1 && len_pow > 0.f, "mrblip_beam_advance: sequence rows of %lld hold no position %d", lds_, cur_len);
  MRB_REQUIRE(cand_score && cand_index && seq_in && seq_out && seq_in != seq_out && beam_scores && parents && tokens && pool_score && pool_len &&
                  pool_seq && pool_n && done && done_count,
              "mrblip_beam_advance: null buffer (or seq_in == seq_out: the sequences ping-pong)");
  AdvanceArgs a = {cand_score, cand_index, seq_in, seq_out, lds_, beam_scores, parents, tokens, pool_score, pool_len, pool_seq, pool_n, done,
                   done_count, K, V, cur_len, eos_id, pad_id, len_pow};
  hipLaunchKernelGGL(beam_advance_kernel, dim3(B), dim3(64), 0, stream, a);
  return mrblip_check_launch("mrblip_beam_advance");
}

extern "C" int mrblip_beam_finalize(const int* seq, long long lds_, const float* beam_scores, float* pool_score, int* pool_len, int* pool_seq,
                                    int* pool_n, const int* done, int B, int K, int cur_len, float len_pow, int num_return, int* out,
                                    hipStream_t stream) {
  MRB_REQUIRE(K >= 1 && K <= BS_MAX_K && B >= 1 && num_return >= 1 && num_return <= K, "mrblip_beam_finalize: B = %d, K = %d (1..%d), num_return = %d (1..K)",
              B, K, BS_MAX_K, num_return);
  MRB_REQUIRE(cur_len >= 1 && lds_ >= cur_len && len_pow > 0.f, "mrblip_beam_finalize: bad cur_len / leading dimension / length term");
  MRB_REQUIRE(seq && beam_scores && pool_score && pool_len && pool_seq && pool_n && done && out, "mrblip_beam_finalize: null buffer");
  hipLaunchKernelGGL(beam_finalize_kernel, dim3(B), dim3(64), 0, stream, seq, lds_, beam_scores, pool_score, pool_len, pool_seq, pool_n, done, K,
                     cur_len, len_pow, num_return, out);
  return mrblip_check_launch("mrblip_beam_finalize");
}

extern "C" int mrblip_kv_gather_rows(const void* src, void* dst, const int* parents, int planes, int R, int Lmax, int inner, int t,
                                     hipStream_t stream) {
  MRB_REQUIRE(planes >= 1 && planes <= 65535 && R >= 1 && Lmax >= 1 && inner >= 8 && inner % 8 == 0 && t >= 0 && t <= Lmax,
              "mrblip_kv_gather_rows: planes = %d, R = %d, Lmax = %d, inner = %d (multiple of 8), t = %d (0..Lmax)", planes, R, Lmax, inner, t);
  MRB_REQUIRE(src && dst && src != dst && parents && ((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0,
              "mrblip_kv_gather_rows: null / unaligned buffer (or src == dst: parents repeat, the copy goes to the other cache buffer)");
  if (t == 0) return MRBLIP_OK;
  const long long row16 = (long long)Lmax * inner / 8, n16 = (long long)t * inner / 8;
  const int nz = (int)((n16 + 2047) / 2048 > 8 ? 8 : (n16 + 2047) / 2048);
  hipLaunchKernelGGL(kv_gather_rows_kernel, dim3(R, planes, nz), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst, parents, R, row16, n16);
  return mrblip_check_launch("mrblip_kv_gather_rows");
}

static int sample_shape_ok(const char* who, int R, int V, int top_k) {
  MRB_REQUIRE(top_k >= 1 && top_k <= SS_MAX_K, "%s: top_k = %d, 1..%d supported", who, top_k, SS_MAX_K);
  MRB_REQUIRE(R >= 1 && R <= SS_MAX_ROWS, "%s: R = %d rows, 1..%d supported", who, R, SS_MAX_ROWS);
  MRB_REQUIRE(V >= 1 && V <= BS_MAX_SPLIT * BS_CHUNK, "%s: V = %d, 1..%d supported", who, V, BS_MAX_SPLIT * BS_CHUNK);
  return MRBLIP_OK;
}

extern "C" long long mrblip_sample_topk_workspace_bytes(int R, int top_k, int V) {
  if (sample_shape_ok("mrblip_sample_topk_workspace_bytes", R, V, top_k) != MRBLIP_OK) return -1;
  const int NS = (V + BS_CHUNK - 1) / BS_CHUNK, k = top_k < V ? top_k : V;
  return 8ll * R * NS * k;
}

extern "C" int mrblip_sample_topk(const float* logits, long long ldl, const int* seqs, long long lds_, int R, int V, int cur_len, int top_k,
                                  int min_length, int eos_id, float repetition_penalty, float* cand_score, int* cand_index, void* ws,
                                  long long ws_bytes, hipStream_t stream) {
  if (sample_shape_ok("mrblip_sample_topk", R, V, top_k) != MRBLIP_OK) return MRBLIP_EINVAL;
  MRB_REQUIRE(cur_len >= 1 && lds_ >= cur_len && ldl >= V && repetition_penalty > 0.f, "mrblip_sample_topk: bad cur_len / leading dimension / penalty");
  const int NS = (V + BS_CHUNK - 1) / BS_CHUNK, k = top_k < V ? top_k : V;
  const long long need = 8ll * R * NS * k;
  MRB_REQUIRE(logits && seqs && cand_score && cand_index && ws && ws_bytes >= need && ((uintptr_t)ws % 16) == 0,
              "mrblip_sample_topk: null buffer or workspace below %lld bytes (8 * R * ceil(V / 2048) * min(top_k, V))", need);
  float* part_s = (float*)ws;
  int* part_i = (int*)(part_s + (long long)R * NS * k);
  hipLaunchKernelGGL(sample_select_kernel, dim3(NS, R), dim3(256), 0, stream, logits, ldl, seqs, lds_, NS, k, V, cur_len, cur_len < min_length ? 1 : 0,
                     eos_id, repetition_penalty, part_s, part_i);
  hipLaunchKernelGGL(sample_merge_kernel, dim3(R), dim3(64), 0, stream, part_s, part_i, NS, k, cand_score, cand_index);
  return mrblip_check_launch("mrblip_sample_topk");
}

extern "C" int mrblip_sample_advance(const float* cand_score, const int* cand_index, int* seq, long long lds_, int* tokens, int* unfinished,
                                     int* length, int* done_count, const float* uniforms, uint32_t seed, int R, int V, int top_k, int cur_len,
                                     int eos_id, int pad_id, float temperature, float top_p, int greedy, hipStream_t stream) {
  if (sample_shape_ok("mrblip_sample_advance", R, V, top_k) != MRBLIP_OK) return MRBLIP_EINVAL;
  MRB_REQUIRE(temperature > 0.f && top_p > 0.f, "mrblip_sample_advance: temperature = %g, top_p = %g (both have to be positive)", (double)temperature,
              (double)top_p);
  MRB_REQUIRE(cur_len >= 1 && lds_ >= cur_len + 1, "mrblip_sample_advance: sequence rows of %lld hold no position %d", lds_, cur_len);
  MRB_REQUIRE(uniforms || cur_len <= 256, "mrblip_sample_advance: the built-in draws cover 256 steps, step %d needs caller-provided uniforms", cur_len - 1);
  MRB_REQUIRE(pad_id >= 0 && pad_id < V, "mrblip_sample_advance: pad_id = %d outside the vocabulary of %d", pad_id, V);
  MRB_REQUIRE(cand_score && cand_index && seq && tokens && unfinished && length && done_count, "mrblip_sample_advance: null buffer");
  SampleArgs a = {cand_score, cand_index, seq, lds_, tokens, unfinished, length, done_count, uniforms, seed, R, V, top_k < V ? top_k : V, cur_len, eos_id,
                  pad_id, greedy ? 1 : 0, temperature, top_p};
  hipLaunchKernelGGL(sample_advance_kernel, dim3(1), dim3(SS_MAX_ROWS), 0, stream, a);
  return mrblip_check_launch("mrblip_sample_advance");
}
