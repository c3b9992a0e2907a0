// Train-split augmentation on the device (gfx950): the crop + bicubic resize of Blip2VideoTrainProcessor's RandomResizedCropVideo
// — one box per clip, shared by its frames — on uint8 frames that were uploaded uncropped.  Same arithmetic as the loader's CPU path
// (lavis/datasets/data_utils.py: random_resized_crop_u8): torch's upsample_bicubic2d with align_corners=False on the CROP (taps
// clamped to the crop, not the frame), cubic-convolution weights with A = -0.75, fp32 accumulation, clamp to [0, 255] BEFORE the
// truncating cast (the documented deviation from the reference's wrapping cast).
//
// Source position of output index o along an axis of `in` source and `out` output pixels: s = (in / out) * (o + 0.5) - 0.5 =
// (in * (2 o + 1) - out) / (2 out).  The integer form gives floor(s) exactly and the fraction t as ONE correctly rounded division
// of two small integers; s evaluated in fp32 would carry half an ulp of up to 4096 (2.4e-4) into t, i.e. ~0.05 grey levels.
// t = 0 gives the weights (0, 1, 0, 0) exactly, so a full-frame box with H = W = OUT copies the frame bit for bit; a constant image
// comes back as the constant for any box (cubic_mix below).
//
// Shape: one workgroup = CR_BAND output rows of one channel plane.  Each wave takes source rows of the band round-robin: it loads
// the row's crop window with aligned 4-byte loads (64 lanes x 4 B, coalesced) into its own LDS line, then runs the horizontal pass
// (4 taps from that line, weights from an LDS table built once per workgroup) into an fp32 LDS tile [source row][OUT].  After one
// barrier the vertical pass reads 4 rows x 16 B per lane from the tile, clamps, packs four uint8 and stores 4 B per lane, coalesced.
// A band that needs more source rows than the tile holds (strong down-scale) is walked in sub-bands.  No atomics, no scratch, and
// every output byte has one writer with a fixed summation order: the same bits on every run.
#include "common.h"
#include "../../include/mrblip_hip.h"

#define CR_MAX_CLIPS 64
#define CR_BAND 16
#define CR_THREADS 256
#define CR_WAVES (CR_THREADS / 64)
#define CR_LDS_BYTES (64 * 1024)

struct CropBoxes {
  int v[CR_MAX_CLIPS][4];  // (i, j, h, w) per clip: top, left, height, width
};

// cubic-convolution weights of the taps i0-1 .. i0+2 at fraction t (A = -0.75), the polynomials as torch's UpSample.h writes them
__device__ __forceinline__ float4 cubic_weights(float t) {
  const float A = -0.75f;
  float4 w;
  float x = t + 1.0f;
  w.x = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  x = t;
  w.y = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 1.0f - t;
  w.z = ((A + 2.0f) * x - (A + 3.0f)) * x * x + 1.0f;
  x = 2.0f - t;
  w.w = ((A * x - 5.0f * A) * x + 8.0f * A) * x - 4.0f * A;
  return w;
}

// w.x a0 + w.y a1 + w.z a2 + w.w a3 with w.y = 1 - (w.x + w.z + w.w) folded in (the four weights sum to one): the taps enter as differences
// from the nearest one, so a constant neighbourhood returns the constant exactly — four rounded products of a constant can sum to
// c - 1 ulp, which the truncating cast would turn into c - 1 — and t = 0 (weights 0, 1, 0, 0) returns a1 exactly.
__device__ __forceinline__ float cubic_mix(float4 w, float a0, float a1, float a2, float a3) {
  return a1 + (w.x * (a0 - a1) + w.z * (a2 - a1) + w.w * (a3 - a1));
}

// floor(s) and s - floor(s) of s = (in / out) * (o + 0.5) - 0.5, exact up to the one rounding of the division (operands < 2^24)
__device__ __forceinline__ void src_pos(int o, int in, int out, int& i0, float& t) {
  const int num = in * (2 * o + 1) - out, den = 2 * out;
  int q = num / den, r = num - q * den;
  if (r < 0) {
    r += den;
    --q;
  }
  i0 = q;
  t = (float)r / (float)den;
}

// orders one wave's LDS writes before its own later LDS reads of other lanes' data (the LDS serves a wave's accesses in order)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ uint32_t clamp_u8(float v) { return (uint32_t)__builtin_amdgcn_fmed3f(v, 0.0f, 255.0f); }

__global__ __launch_bounds__(CR_THREADS) void crop_resize_u8_kernel(const uint8_t* __restrict__ src, long long src_bytes, int H, int W, CropBoxes boxes,
                                                                    int frames_per_clip, uint8_t* __restrict__ dst, int OUT, int OUTp, int R,
                                                                    int raw_stride, int vec_store) {
  extern __shared__ __align__(16) unsigned char cr_smem[];
  float4* xw = reinterpret_cast<float4*>(cr_smem);                  // [OUTp]     horizontal weights per output column
  float4* yw = xw + OUTp;                                           // [CR_BAND]  vertical weights per output row of the band
  float* hbuf = reinterpret_cast<float*>(yw + CR_BAND);             // [R][OUTp]  horizontally resampled source rows
  int* xi = reinterpret_cast<int*>(hbuf + (size_t)R * OUTp);        // [OUTp]     floor(source x) per output column
  int* yi = xi + OUTp;                                              // [CR_BAND]
  unsigned char* raw = reinterpret_cast<unsigned char*>(yi + CR_BAND);  // [CR_WAVES][raw_stride] one source row per wave

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int plane = blockIdx.y;                                     // frame * 3 + channel
  const int* box = boxes.v[(plane / 3) / frames_per_clip];
  const int bi = box[0], bj = box[1], bh = box[2], bw = box[3];
  const int y_beg = blockIdx.x * CR_BAND, y_end = min(OUT, y_beg + CR_BAND);

  for (int x = tid; x < OUT; x += CR_THREADS) {
    int i0;
    float t;
    src_pos(x, bw, OUT, i0, t);
    xw[x] = cubic_weights(t);
    xi[x] = i0;
  }
  if (tid < y_end - y_beg) {
    int i0;
    float t;
    src_pos(y_beg + tid, bh, OUT, i0, t);
    yw[tid] = cubic_weights(t);
    yi[tid] = i0;
  }
  __syncthreads();

  const uint8_t* plane_src = src + (long long)plane * H * W;
  const uint8_t* src_end = src + src_bytes;
  uint8_t* plane_dst = dst + (long long)plane * OUT * OUT;
  unsigned char* my_raw = raw + wv * raw_stride;
  const int nx4 = OUTp >> 2;

  int y0 = y_beg;
  while (y0 < y_end) {  // sub-bands: output rows [y0, y1) whose source rows [lo, hi] fit the tile (every value here is block-uniform)
    const int lo = max(yi[y0 - y_beg] - 1, 0);
    int y1 = y0 + 1;
    while (y1 < y_end && min(yi[y1 - y_beg] + 2, bh - 1) - lo + 1 <= R) ++y1;
    const int hi = min(yi[y1 - 1 - y_beg] + 2, bh - 1);

    for (int r = lo + wv; r <= hi; r += CR_WAVES) {
      const uint8_t* p = plane_src + (long long)(bi + r) * W + bj;
      const int mis = (int)(reinterpret_cast<uintptr_t>(p) & 3);
      const uint8_t* p4 = p - mis;                                   // src is 4-B aligned (host check): never below the buffer
      const int ndw = (mis + bw + 3) >> 2;
      for (int d = lane; d < ndw; d += 64) {
        const uint8_t* q = p4 + 4 * d;
        uint32_t v;
        if (q + 4 <= src_end) {
          v = *reinterpret_cast<const uint32_t*>(q);
        } else {                                                     // the buffer's last, partial dword
          v = 0;
          for (int k = 0; k < 4; ++k)
            if (q + k < src_end) v |= (uint32_t)q[k] << (8 * k);
        }
        reinterpret_cast<uint32_t*>(my_raw)[d] = v;
      }
      wave_lds_sync();
      const unsigned char* rp = my_raw + mis;
      float* hrow = hbuf + (size_t)(r - lo) * OUTp;
      for (int x = lane; x < OUT; x += 64) {
        const float4 w = xw[x];
        const int i0 = xi[x];
        const float a0 = (float)rp[min(max(i0 - 1, 0), bw - 1)], a1 = (float)rp[min(max(i0, 0), bw - 1)];
        const float a2 = (float)rp[min(i0 + 1, bw - 1)], a3 = (float)rp[min(i0 + 2, bw - 1)];
        hrow[x] = cubic_mix(w, a0, a1, a2, a3);
      }
      wave_lds_sync();                                               // the next row overwrites my_raw
    }
    __syncthreads();

    const int items = (y1 - y0) * nx4;
    for (int it = tid; it < items; it += CR_THREADS) {
      const int yl = y0 - y_beg + it / nx4, x = (it % nx4) * 4;
      const float4 w = yw[yl];
      const int i0 = yi[yl];
      const float4 r0 = *reinterpret_cast<const float4*>(hbuf + (size_t)(min(max(i0 - 1, 0), bh - 1) - lo) * OUTp + x);
      const float4 r1 = *reinterpret_cast<const float4*>(hbuf + (size_t)(min(max(i0, 0), bh - 1) - lo) * OUTp + x);
      const float4 r2 = *reinterpret_cast<const float4*>(hbuf + (size_t)(min(i0 + 1, bh - 1) - lo) * OUTp + x);
      const float4 r3 = *reinterpret_cast<const float4*>(hbuf + (size_t)(min(i0 + 2, bh - 1) - lo) * OUTp + x);
      const uint32_t b0 = clamp_u8(cubic_mix(w, r0.x, r1.x, r2.x, r3.x));
      const uint32_t b1 = clamp_u8(cubic_mix(w, r0.y, r1.y, r2.y, r3.y));
      const uint32_t b2 = clamp_u8(cubic_mix(w, r0.z, r1.z, r2.z, r3.z));
      const uint32_t b3 = clamp_u8(cubic_mix(w, r0.w, r1.w, r2.w, r3.w));
      uint8_t* o = plane_dst + (long long)(y_beg + yl) * OUT + x;
      if (vec_store) {
        *reinterpret_cast<uint32_t*>(o) = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
      } else {                                                       // OUT % 4 != 0 or an unaligned dst: byte stores, columns >= OUT dropped
        o[0] = (uint8_t)b0;
        if (x + 1 < OUT) o[1] = (uint8_t)b1;
        if (x + 2 < OUT) o[2] = (uint8_t)b2;
        if (x + 3 < OUT) o[3] = (uint8_t)b3;
      }
    }
    __syncthreads();                                                 // the next sub-band overwrites the tile
    y0 = y1;
  }
}

extern "C" int mrblip_crop_resize_u8(const uint8_t* src, int F, int H, int W, const int* boxes_host, int n_clips, int frames_per_clip, uint8_t* dst,
                                     int OUT, hipStream_t stream) {
  MRB_REQUIRE(src && dst && boxes_host, "crop_resize_u8: null pointer");
  MRB_REQUIRE(n_clips >= 1 && n_clips <= CR_MAX_CLIPS, "crop_resize_u8: n_clips = %d, expected 1 .. %d (the boxes travel in the kernel arguments)", n_clips,
              CR_MAX_CLIPS);
  MRB_REQUIRE(F >= 1 && frames_per_clip >= 1 && (long long)n_clips * frames_per_clip == F, "crop_resize_u8: F = %d is not n_clips * frames_per_clip = %d * %d", F,
              n_clips, frames_per_clip);
  MRB_REQUIRE(H >= 1 && W >= 1 && H <= 4096 && W <= 4096, "crop_resize_u8: frame %d x %d, expected 1 .. 4096 per side", H, W);
  MRB_REQUIRE(OUT >= 1 && OUT <= 1024, "crop_resize_u8: OUT = %d, expected 1 .. 1024", OUT);
  MRB_REQUIRE(3ll * F <= 65535, "crop_resize_u8: %d frames exceed the grid (21845)", F);
  MRB_REQUIRE(((uintptr_t)src % 4) == 0, "crop_resize_u8: src must be 4-B aligned");
  CropBoxes boxes = {};
  int hmax = 1, wmax = 1;
  for (int c = 0; c < n_clips; ++c) {
    const int i = boxes_host[4 * c], j = boxes_host[4 * c + 1], h = boxes_host[4 * c + 2], w = boxes_host[4 * c + 3];
    MRB_REQUIRE(h >= 1 && w >= 1, "crop_resize_u8: box %d has height %d, width %d (need >= 1)", c, h, w);
    MRB_REQUIRE(i >= 0 && j >= 0 && h <= H && w <= W && i <= H - h && j <= W - w, "crop_resize_u8: box %d (i %d, j %d, h %d, w %d) leaves the %d x %d frame", c, i, j,
                h, w, H, W);
    boxes.v[c][0] = i, boxes.v[c][1] = j, boxes.v[c][2] = h, boxes.v[c][3] = w;
    hmax = h > hmax ? h : hmax;
    wmax = w > wmax ? w : wmax;
  }
  const int OUTp = (OUT + 3) & ~3;
  const int raw_stride = ((wmax + 6) / 4 + 1) * 4;                   // up to 3 B of misalignment in front, rounded up to whole dwords
  const int fixed = (OUTp + CR_BAND) * (16 + 4) + CR_WAVES * raw_stride;
  const int rows_fit = (CR_LDS_BYTES - fixed) / (OUTp * 4);
  int rows_band = ((CR_BAND - 1) * hmax + OUT - 1) / OUT + 4;        // source rows a whole band touches
  rows_band = rows_band < hmax ? rows_band : hmax;
  const int R = rows_band < rows_fit ? rows_band : rows_fit;         // fewer than the band needs: the kernel walks sub-bands
  MRB_REQUIRE(R >= (hmax < 4 ? hmax : 4), "crop_resize_u8: the staging tile cannot hold the four source rows of one output row");
  const int vec_store = (OUT % 4 == 0 && ((uintptr_t)dst % 4) == 0) ? 1 : 0;
  const size_t lds = (size_t)fixed + (size_t)R * OUTp * 4;
  hipLaunchKernelGGL(crop_resize_u8_kernel, dim3((OUT + CR_BAND - 1) / CR_BAND, 3 * F), dim3(CR_THREADS), lds, stream, src, (long long)F * 3 * H * W, H, W, boxes,
                     frames_per_clip, dst, OUT, OUTp, R, raw_stride, vec_store);
  return mrblip_check_launch("crop_resize_u8");
}
