// Single-query self-attention of generate's decode step against the ROW-MAJOR K / V cache of t5_decode_begin
// ([2 (k, v), layers, R, Lmax, H * D] bf16): one launch per decoder layer re-orders the cache rows by beam parent while it reads them,
// appends the new position's K / V from the layer's qkv projection and attends the one query to positions 0..pos.  The position is a
// host int or a device word, so the launch has no shape, stride or pointer that depends on it (a captured step can be replayed).
//
// Mapping: a workgroup of 256 lanes owns one (row, head).  The work is at most Lmax keys x 128 dims — latency, not arithmetic — so K and V
// go straight from memory to registers, 16 bytes per lane: 8 lanes share a key (chunks of 8 dims, two chunks per lane above D = 64), a wave
// covers 8 keys per load instruction and the workgroup 32.  Scores and probabilities live in LDS (Lmax floats).  Every reduction is a
// fixed butterfly / fixed-order sum, nothing is atomic: two launches give the same bits.
#include "common.h"
#include "../../include/mrblip_hip.h"
#include <math.h>

#define DSA_MAX_LMAX 8192   // scores in LDS: 32 KB
#define DSA_MAX_D 128
#define DSA_LDS_EXTRA (8 + 4 * 16 * 8)   // floats behind the scores: max / sum partials of the 4 waves, output partials [wave][chunk][8]

namespace {

struct DecodeArgs {
  const bf16_t* kv_src;
  bf16_t* kv_dst;
  const bf16_t* qkv;
  long long ldq;
  bf16_t* out;
  long long ldo;
  const float* lut;
  const int* parents;
  const int* pos_dev;
  int pos;
  float scale;
  int R, H, D, Lmax;
  long long plane;       // elements between the K and the V plane: layers * R * Lmax * inner
  long long layer_off;   // layer * R * Lmax * inner
};

__device__ __forceinline__ void unpack8(const uint4 v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}

// NC: 8-dim chunks per lane (1: D <= 64, 2: D <= 128)
template <int NC>
__global__ __launch_bounds__(256) void decode_self_attn_kernel(const DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) float dsa_lds[];
  const int h = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
  const int pos = a.pos_dev ? *a.pos_dev : a.pos;
  if (pos < 0 || pos >= a.Lmax) return;   // (device form: before the first store)
  const bool reorder = a.parents != nullptr;
  int p = r;
  if (reorder) {
    p = a.parents[r];
    if (p < 0 || p >= a.R) p = r;   // (never read outside the cache, whatever the index buffer holds)
  }
  const int D = a.D, inner = a.H * D, nchunk = D >> 3;
  const int c = tid & 7, kg = tid >> 3, wave = tid >> 6, lane = tid & 63;
  float* sc = dsa_lds;
  float* red = dsa_lds + a.Lmax;
  float* part = red + 8;

  const bf16_t* qrow = a.qkv + (long long)r * a.ldq + h * D;   // q; + inner: the new K row; + 2 * inner: the new V row
  const long long row_src = a.layer_off + (long long)p * a.Lmax * inner + h * D;
  const long long row_dst = a.layer_off + (long long)r * a.Lmax * inner + h * D;
  const bf16_t* ksrc = a.kv_src + row_src;
  const bf16_t* vsrc = a.kv_src + a.plane + row_src;
  bf16_t* kdst = a.kv_dst + row_dst;
  bf16_t* vdst = a.kv_dst + a.plane + row_dst;

  float q[NC][8];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int ch = c + 8 * i;
    uint4 v = {0u, 0u, 0u, 0u};
    if (ch < nchunk) v = *reinterpret_cast<const uint4*>(qrow + ch * 8);
    unpack8(v, q[i]);
  }

  // ---- scores: key j = kg + 32 * it, the 8 lanes of a key each dot their chunk(s)
  for (int j = kg; j <= pos; j += 32) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int ch = c + 8 * i;
      if (ch < nchunk) {
        const uint4 kk = j == pos ? *reinterpret_cast<const uint4*>(qrow + inner + ch * 8)
                                  : *reinterpret_cast<const uint4*>(ksrc + (long long)j * inner + ch * 8);
        if (reorder || j == pos) *reinterpret_cast<uint4*>(kdst + (long long)j * inner + ch * 8) = kk;
        float kf[8];
        unpack8(kk, kf);
#pragma unroll
        for (int e = 0; e < 8; ++e) s += q[i][e] * kf[e];
      }
    }
    s += __shfl_xor(s, 1, 64);
    s += __shfl_xor(s, 2, 64);
    s += __shfl_xor(s, 4, 64);
    if (c == 0) {
      int rel = j - pos;
      rel = rel < -128 ? -128 : (rel > 128 ? 128 : rel);
      sc[j] = s * a.scale + a.lut[h * 257 + rel + 128];
    }
  }
  __syncthreads();

  // ---- softmax over sc[0..pos] in fp32
  float m = -INFINITY;
  for (int j = tid; j <= pos; j += 256) m = fmaxf(m, sc[j]);
  m = wave_max(m);
  if (lane == 0) red[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  float l = 0.f;
  for (int j = tid; j <= pos; j += 256) {
    const float e = expf(sc[j] - m);
    sc[j] = e;
    l += e;
  }
  l = wave_sum(l);
  if (lane == 0) red[4 + wave] = l;
  __syncthreads();
  l = (red[4] + red[5]) + (red[6] + red[7]);

  // ---- o = sum_j p_j v_j: per lane over its keys, then over the 8 key groups of the wave, then over the 4 waves
  float acc[NC][8];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
  for (int j = kg; j <= pos; j += 32) {
    const float w = sc[j];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int ch = c + 8 * i;
      if (ch < nchunk) {
        const uint4 vv = j == pos ? *reinterpret_cast<const uint4*>(qrow + 2 * inner + ch * 8)
                                  : *reinterpret_cast<const uint4*>(vsrc + (long long)j * inner + ch * 8);
        if (reorder || j == pos) *reinterpret_cast<uint4*>(vdst + (long long)j * inner + ch * 8) = vv;
        float vf[8];
        unpack8(vv, vf);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] += w * vf[e];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = acc[i][e];
      v += __shfl_xor(v, 8, 64);
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      acc[i][e] = v;
    }
  if (lane < 8) {
#pragma unroll
    for (int i = 0; i < NC; ++i) {
      const int ch = c + 8 * i;
      if (ch < nchunk) {
#pragma unroll
        for (int e = 0; e < 8; ++e) part[(wave * 16 + ch) * 8 + e] = acc[i][e];
      }
    }
  }
  __syncthreads();
  if (tid < nchunk) {
    const float inv = 1.0f / l;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e)
      o[e] = ((part[(0 * 16 + tid) * 8 + e] + part[(1 * 16 + tid) * 8 + e]) + (part[(2 * 16 + tid) * 8 + e] + part[(3 * 16 + tid) * 8 + e])) * inv;
    uint4 v;
    v.x = pack2bf(o[0], o[1]);
    v.y = pack2bf(o[2], o[3]);
    v.z = pack2bf(o[4], o[5]);
    v.w = pack2bf(o[6], o[7]);
    *reinterpret_cast<uint4*>(a.out + (long long)r * a.ldo + h * D + tid * 8) = v;
  }
}

}  // namespace

extern "C" int mrblip_decode_self_attention(const void* kv_src, void* kv_dst, const void* qkv, long long ldq, void* out, long long ldo,
                                            const float* lut, const int* parents, const int* pos_dev, int pos, int layers, int layer, int R,
                                            int Lmax, int H, int D, float scale, hipStream_t stream) {
  MRB_REQUIRE(R >= 1 && R <= 65535 && H >= 1 && H <= 65535 && Lmax >= 1 && Lmax <= DSA_MAX_LMAX,
              "mrblip_decode_self_attention: R = %d, H = %d (1..65535), Lmax = %d (1..%d)", R, H, Lmax, DSA_MAX_LMAX);
  MRB_REQUIRE(D >= 8 && D <= DSA_MAX_D && D % 8 == 0, "mrblip_decode_self_attention: D = %d, multiples of 8 up to %d supported", D, DSA_MAX_D);
  MRB_REQUIRE(layers >= 1 && layer >= 0 && layer < layers, "mrblip_decode_self_attention: layer = %d outside 0..%d", layer, layers - 1);
  MRB_REQUIRE(pos_dev != nullptr || (pos >= 0 && pos < Lmax), "mrblip_decode_self_attention: pos = %d outside 0..Lmax-1 = %d", pos, Lmax - 1);
  const long long inner = (long long)H * D;
  MRB_REQUIRE(ldq >= 3 * inner && ldo >= inner && ldq % 8 == 0 && ldo % 8 == 0,
              "mrblip_decode_self_attention: ldq = %lld (>= 3 * H * D = %lld), ldo = %lld (>= H * D), both multiples of 8", ldq, 3 * inner, ldo);
  MRB_REQUIRE(kv_src && kv_dst && qkv && out && lut, "mrblip_decode_self_attention: null buffer");
  MRB_REQUIRE(parents ? kv_src != kv_dst : kv_src == kv_dst,
              "mrblip_decode_self_attention: with parents the re-ordered cache goes to the OTHER buffer (kv_src != kv_dst: parents repeat), "
              "without parents the cache is used in place (kv_src == kv_dst)");
  MRB_REQUIRE(((uintptr_t)kv_src % 16) == 0 && ((uintptr_t)kv_dst % 16) == 0 && ((uintptr_t)qkv % 16) == 0 && ((uintptr_t)out % 16) == 0 &&
                  ((uintptr_t)lut % 4) == 0 && ((uintptr_t)parents % 4) == 0 && ((uintptr_t)pos_dev % 4) == 0,
              "mrblip_decode_self_attention: unaligned buffer (cache, qkv and out: 16 bytes)");
  DecodeArgs a;
  a.kv_src = (const bf16_t*)kv_src;
  a.kv_dst = (bf16_t*)kv_dst;
  a.qkv = (const bf16_t*)qkv;
  a.ldq = ldq;
  a.out = (bf16_t*)out;
  a.ldo = ldo;
  a.lut = lut;
  a.parents = parents;
  a.pos_dev = pos_dev;
  a.pos = pos;
  a.scale = scale;
  a.R = R;
  a.H = H;
  a.D = D;
  a.Lmax = Lmax;
  a.plane = (long long)layers * R * Lmax * inner;
  a.layer_off = (long long)layer * R * Lmax * inner;
  const int lds = (Lmax + DSA_LDS_EXTRA) * 4, lds_max = (DSA_MAX_LMAX + DSA_LDS_EXTRA) * 4;
  const dim3 grid(H, R), block(256);
  if (D <= 64) return mrb_launch_lds<decode_self_attn_kernel<1>>("mrblip_decode_self_attention", lds_max, grid, block, lds, stream, a);
  return mrb_launch_lds<decode_self_attn_kernel<2>>("mrblip_decode_self_attention", lds_max, grid, block, lds, stream, a);
}
