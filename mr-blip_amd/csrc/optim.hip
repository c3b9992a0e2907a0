// The gradient guard of the optimizer step: global gradient norm, non-finite check, clipping by global norm and the
// optimizer clock, all decided on the device in two launches in front of the unchanged adamw_kernel (elementwise.hip):
//   (a) grad_sumsq_kernel     one record {fp64 sum of squares, count of non-finite values} per FIXED chunk of the flat fp32 gradient
//   (b) optim_prepare_kernel  one workgroup: adds the records in chunk order, decides apply / skip, counts the step, writes AdamW's hyper block
// No atomics, tickets or flags: (b) starts after (a) by stream order (the store pass + sum pass form).  Every addition is fp64 in an order
// fixed by the element index and by g's position inside its 16-byte line — never by the grid, the CU count or the run; the square of an
// fp32 value is exact in fp64 (24-bit x 24-bit mantissa), so a record is the correctly accumulated fp64 sum of exact terms.
// The library keeps no state of its own: records, state block and hyper blocks are the caller's device memory.
#include "common.h"
#include <math.h>

#define OPT_CHUNK 16384          // elements per record: chunk c is ALWAYS [c * OPT_CHUNK, min((c + 1) * OPT_CHUNK, n)), whatever the grid
#define OPT_MAX_GRID 2048
#define OPT_STATE_WORDS 8        // state block (include/mrblip_hip.h): skip, applied, skipped, nonfinite, norm, clip, consecutive_skips, reserved
#define OPT_TILE 1024            // records staged in LDS per pass of the prepare kernel

namespace {

struct OptRecord {
  double sumsq;                  // sum of (double)g[i] * (double)g[i] over the chunk's FINITE values
  uint32_t nonfinite;            // inf / nan values of the chunk
  uint32_t reserved;
};
static_assert(sizeof(OptRecord) == 16, "record layout is part of the documented workspace");

__device__ __forceinline__ void opt_acc(float x, double& s, uint32_t& c) {
  const bool bad = (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u;   // exponent all ones: inf or nan
  const double d = (double)x;
  s += bad ? 0.0 : d * d;        // (contracted to an fma or not: d * d is exact, so both forms round the same sum once)
  c += bad ? 1u : 0u;
}

// A chunk is read as: up to 3 scalar head elements (to the next 16-byte line of the ADDRESS — g may start at any 4-byte-aligned address,
// the decay / no-decay segments are slices of one buffer), 16-byte vectors, up to 3 scalar tail elements.  Nothing outside [g, g + n)
// is touched.  Thread t owns head element t, vectors t, t + 256, ..., tail element t, added in that order; then a butterfly over the
// wave (both partners add the same two values: every lane ends with the same bits), then the four waves in index order.
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, long long n, OptRecord* __restrict__ rec, long long nchunks) {
  __shared__ double wave_s[4];
  __shared__ uint32_t wave_c[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const float* gc = g + c * OPT_CHUNK;
    const long long rem = n - c * OPT_CHUNK;
    const int L = rem < OPT_CHUNK ? (int)rem : OPT_CHUNK;
    int head = (int)((16u - (uint32_t)((uintptr_t)gc & 15u)) & 15u) >> 2;
    if (head > L) head = L;
    const int nv = (L - head) >> 2, tail_at = head + 4 * nv, tail = L - tail_at;
    double s = 0.0;
    uint32_t cnt = 0u;
    if (t < head) opt_acc(gc[t], s, cnt);
    const float4* gv = reinterpret_cast<const float4*>(gc + head);
#pragma unroll 8
    for (int i = t; i < nv; i += 256) {
      const float4 q = gv[i];
      opt_acc(q.x, s, cnt);
      opt_acc(q.y, s, cnt);
      opt_acc(q.z, s, cnt);
      opt_acc(q.w, s, cnt);
    }
    if (t < tail) opt_acc(gc[tail_at + t], s, cnt);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      s += __shfl_xor(s, o, 64);
      cnt += __shfl_xor(cnt, o, 64);
    }
    if (lane == 0) { wave_s[wave] = s; wave_c[wave] = cnt; }
    __syncthreads();
    if (t == 0) {
      OptRecord r;
      r.sumsq = ((wave_s[0] + wave_s[1]) + wave_s[2]) + wave_s[3];
      r.nonfinite = wave_c[0] + wave_c[1] + wave_c[2] + wave_c[3];
      r.reserved = 0u;
      rec[c] = r;
    }
    __syncthreads();
  }
}

// One workgroup.  The records pass through LDS OPT_TILE at a time (coalesced reads by all threads); thread 0 adds them in chunk order.
__global__ __launch_bounds__(256) void optim_prepare_kernel(const OptRecord* __restrict__ rec, long long nchunks, const float* __restrict__ hyper_in,
                                                            double beta1, double beta2, float max_norm, const uint32_t* __restrict__ guard_in,
                                                            uint32_t* __restrict__ state, float* __restrict__ hyper_out) {
  __shared__ double tile_s[OPT_TILE];
  __shared__ uint32_t tile_c[OPT_TILE];
  const int t = threadIdx.x;
  double S = 0.0;
  unsigned long long bad = 0ull;
  for (long long base = 0; base < nchunks; base += OPT_TILE) {
    const int m = nchunks - base < OPT_TILE ? (int)(nchunks - base) : OPT_TILE;
    for (int i = t; i < m; i += 256) {
      const OptRecord r = rec[base + i];
      tile_s[i] = r.sumsq;
      tile_c[i] = r.nonfinite;
    }
    __syncthreads();
    if (t == 0)
      for (int i = 0; i < m; ++i) { S += tile_s[i]; bad += tile_c[i]; }
    __syncthreads();
  }
  if (t != 0) return;
  const float lr = hyper_in[0], gs = hyper_in[1];
  const double norm_d = fabs((double)gs) * sqrt(S);
  float norm = (float)norm_d;                                   // a norm beyond fp32 rounds to +inf: counts as non-finite
  if (bad != 0ull) norm = __uint_as_float(0x7f800000u);
  const bool norm_ok = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
  const bool skip = bad != 0ull || !norm_ok || (guard_in != nullptr && *guard_in != 0u);
  uint32_t applied = state[1], skipped = state[2], consecutive = state[6];
  float clip = 1.0f;
  if (!skip) {
    applied += 1u;
    consecutive = 0u;
    const double tt = (double)applied;
    if (max_norm > 0.0f) {
      const double c = (double)max_norm / (norm_d + 1e-6);      // torch.nn.utils.clip_grad_norm_
      clip = c < 1.0 ? (float)c : 1.0f;
    }
    hyper_out[0] = lr;
    hyper_out[1] = (float)(1.0 / (1.0 - pow(beta1, tt)));
    hyper_out[2] = (float)(1.0 / sqrt(1.0 - pow(beta2, tt)));
    hyper_out[3] = gs * clip;
  } else {
    skipped += 1u;
    consecutive += 1u;
    hyper_out[0] = lr; hyper_out[1] = 0.f; hyper_out[2] = 0.f; hyper_out[3] = 0.f;   // (unspecified by contract: the guarded AdamW never reads it)
  }
  state[0] = skip ? 1u : 0u;
  state[1] = applied;
  state[2] = skipped;
  state[3] = bad > 0xffffffffull ? 0xffffffffu : (uint32_t)bad;
  state[4] = __float_as_uint(norm);
  state[5] = __float_as_uint(clip);
  state[6] = consecutive;
  state[7] = 0u;
}

long long opt_chunks(long long n) { return (n + OPT_CHUNK - 1) / OPT_CHUNK; }

}  // namespace

// ========================================================================================================= C ABI
extern "C" long long mrblip_grad_stats_workspace_bytes(long long n) {
  if (n < 0) return -1;
  const long long c = opt_chunks(n);
  return (long long)sizeof(OptRecord) * (c < 1 ? 1 : c);
}

extern "C" int mrblip_grad_sumsq(const float* g, long long n, void* ws, long long ws_bytes, hipStream_t stream) {
  MRB_REQUIRE(n >= 0, "mrblip_grad_sumsq: n = %lld < 0", n);
  MRB_REQUIRE((g || n == 0) && ws, "mrblip_grad_sumsq: null operand");
  MRB_REQUIRE(ws_bytes >= mrblip_grad_stats_workspace_bytes(n), "mrblip_grad_sumsq: workspace of %lld bytes, %lld needed for n = %lld", ws_bytes,
              mrblip_grad_stats_workspace_bytes(n), n);
  MRB_REQUIRE(((uintptr_t)g % 4) == 0 && ((uintptr_t)ws % 16) == 0, "mrblip_grad_sumsq: unaligned buffer (g: 4 bytes, workspace: 16 bytes)");
  if (n == 0) return MRBLIP_OK;
  const long long nchunks = opt_chunks(n);
  const int grid = (int)(nchunks < OPT_MAX_GRID ? nchunks : OPT_MAX_GRID);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3(grid), dim3(256), 0, stream, g, n, (OptRecord*)ws, nchunks);
  return mrblip_check_launch("mrblip_grad_sumsq");
}

extern "C" int mrblip_optim_prepare(const void* ws, long long n, const float* hyper_in, double beta1, double beta2, float max_norm,
                                    const uint32_t* guard_in, void* state, float* hyper_out, hipStream_t stream) {
  MRB_REQUIRE(n >= 0, "mrblip_optim_prepare: n = %lld < 0", n);
  MRB_REQUIRE(ws && hyper_in && state && hyper_out, "mrblip_optim_prepare: null operand");
  MRB_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "mrblip_optim_prepare: beta1 = %g, beta2 = %g outside [0, 1)", beta1, beta2);
  MRB_REQUIRE(max_norm == max_norm, "mrblip_optim_prepare: max_norm is NaN");
  MRB_REQUIRE(((uintptr_t)ws % 16) == 0 && ((uintptr_t)hyper_in % 4) == 0 && ((uintptr_t)guard_in % 4) == 0 && ((uintptr_t)state % 4) == 0 &&
                  ((uintptr_t)hyper_out % 4) == 0,
              "mrblip_optim_prepare: unaligned buffer (workspace: 16 bytes, the others: 4 bytes)");
  hipLaunchKernelGGL(optim_prepare_kernel, dim3(1), dim3(256), 0, stream, (const OptRecord*)ws, opt_chunks(n), hyper_in, beta1, beta2, max_norm, guard_in,
                     (uint32_t*)state, hyper_out);
  return mrblip_check_launch("mrblip_optim_prepare");
}
