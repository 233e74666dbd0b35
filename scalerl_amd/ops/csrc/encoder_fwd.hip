// Fused Atari encoder forward: the three Nature-CNN convolutions of one
// image run back to back in one workgroup, with every intermediate in LDS.
//
//   x  [N,4,84,84] u8 -> /255 -> conv 8x8 s4 +b1, ReLU -> out1 [N,32,20,20]
//                               conv 4x4 s2 +b2, ReLU -> out2 [N,64,9,9]
//                               conv 3x3 s1 +b3, ReLU -> out3 [N,64,7,7]
//
// HBM traffic per image is the 28 KB of bytes in and the 6.3 KB of out3 out;
// the SAVE variant also streams out1 and out2 for the backward pass.  The
// per-layer kernels in conv_fwd.hip move 105 KB per image and re-read every
// weight fragment for every m-tile.
//
// Structure:
//  - persistent workgroups (2 per CU, 4 waves each) stride over the images.
//    Every wave loads the weight (B) fragments of its n-tile for all three
//    layers ONCE, into registers, before the image loop: 8 + 16 + 18
//    fragments = 168 VGPRs.  Weights are never read again.
//  - conv1: the image is staged in two overlapping row ranges (output pixels
//    0..207 need input rows 0..47, pixels 208..399 rows 40..83) with 16-byte
//    global loads, converted to bf16 by frame_cast.h's expression and copied
//    linearly into LDS (pitch 84, no index arithmetic).  25 m-tiles of 16
//    pixels cover the 400 outputs exactly.  The next range's loads are issued
//    before the current range's MFMAs.
//  - each layer's accumulators get bias + ReLU in registers (C/D map: the
//    channel is lane & 15, one bias value per lane) and go straight into the
//    next layer's LDS plane: act1 as NCHW [32][400], act2 channel-last
//    [81][72] so that conv3's A fragments are single 16-byte reads
//    (K order tap*64 + c; conv3's B fragments are gathered to match, once).
//  - conv2 pads 81 pixels to 96 rows and conv3 49 to 64; padded rows read a
//    clamped pixel and are dropped at the store.
//  - LDS: 32256 (image range / act2) + 25600 (act1) + 6272 (out3) = 64128 B,
//    static, two workgroups per CU.
//
// Fragment maps for v_mfma_f32_16x16x32_bf16: mfma.h.

#include "common.h"
#include "frame_cast.h"
#include "mfma.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int ENC_IMG_BYTES = 4 * 84 * 84;  // 28224 = 1764 * 16
constexpr int ENC_CH_EL = 48 * 84;          // LDS elements per input channel
constexpr int ENC_IMG_EL = 4 * ENC_CH_EL;   // 16128 el = 32256 B
constexpr int ENC_ACT1_EL = 32 * 400;       // 12800 el = 25600 B
constexpr int ENC_P3 = 72;                  // act2 pixel pitch (64 ch + 8)
constexpr int ENC_ACT2_EL = 81 * ENC_P3;    // 5832 el, aliases the image
constexpr int ENC_OUT3_EL = 64 * 49;        // 3136 el = 6272 B
static_assert(ENC_ACT2_EL <= ENC_IMG_EL, "act2 aliases the image range");
static_assert((ENC_IMG_EL + ENC_ACT1_EL + ENC_OUT3_EL) * 2 <= 65536,
              "static LDS cap");

// Row range H of the image: H=0 rows 0..47 (output pixels 0..207, m-tiles
// 0..12), H=1 rows 40..83 (pixels 208..399, m-tiles 13..24).  A channel's
// range is contiguous and a multiple of 16 bytes from a 16-byte aligned start.
template <int H>
struct Half {
  static constexpr int R0 = H ? 40 : 0;
  static constexpr int NROWS = H ? 44 : 48;
  static constexpr int VEC = NROWS * 84 / 16;  // 231 / 252 loads per channel
  static constexpr int TILE0 = H ? 13 : 0;
  static constexpr int NTILES = H ? 12 : 13;
  static_assert(NROWS * 84 % 16 == 0 && R0 * 84 % 16 == 0, "16-byte chunks");
  static_assert(VEC <= 256, "one load per thread and channel");
};

template <int H>
__device__ __forceinline__ void load_half(const uint8_t* __restrict__ ximg,
                                          uint4 (&pre)[4], int tid) {
  if (tid < Half<H>::VEC) {
    #pragma unroll
    for (int c = 0; c < 4; ++c)
      pre[c] = reinterpret_cast<const uint4*>(
          ximg + c * (84 * 84) + Half<H>::R0 * 84)[tid];
  }
}

template <int H>
__device__ __forceinline__ void store_half(const uint4 (&pre)[4],
                                           bf16_t* img, int tid) {
  if (tid < Half<H>::VEC) {
    #pragma unroll
    for (int c = 0; c < 4; ++c) {
      uint4 a, b;
      frame_bf16_x16(pre[c], a, b);
      uint4* dst = reinterpret_cast<uint4*>(img + c * ENC_CH_EL);
      dst[2 * tid] = a;
      dst[2 * tid + 1] = b;
    }
  }
}

__device__ __forceinline__ bf16x4 relu_bias_pack(const f32x4 acc, float bias) {
  bf16x4 o;
  #pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (bf16_t)fmaxf(acc[r] + bias, 0.f);
  return o;
}

// conv1 over one row range.  Waves 2*nt and 2*nt+1 share n-tile nt and split
// the m-tiles; each takes two tiles per pass (two independent accumulators).
template <int H>
__device__ __forceinline__ void conv1_half(const bf16_t* img, bf16_t* act1,
                                           const bf16x8 (&B1)[8], float bias,
                                           int wave, int g, int lr) {
  const int nt = wave >> 1;
  for (int t = wave & 1; t < Half<H>::NTILES; t += 4) {
    const bool two = t + 2 < Half<H>::NTILES;          // wave-uniform
    const int tile[2] = {Half<H>::TILE0 + t,
                         Half<H>::TILE0 + (two ? t + 2 : t)};
    int base[2];
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int px = tile[i] * 16 + lr;                // output pixel 0..399
      const int oy = px / 20, ox = px - oy * 20;
      base[i] = (oy * 4 - Half<H>::R0 + g) * 84 + ox * 4;
    }
    f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    #pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
      // k0 = kt*32 + g*8: channel kt>>1, window row (kt&1)*4 + g, 8 px
      const int off = (kt >> 1) * ENC_CH_EL + (kt & 1) * 4 * 84;
      #pragma unroll
      for (int i = 0; i < 2; ++i) {
        const bf16x4* p = reinterpret_cast<const bf16x4*>(img + base[i] + off);
        const bf16x8 a =
            __builtin_shufflevector(p[0], p[1], 0, 1, 2, 3, 4, 5, 6, 7);
        acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, B1[kt], acc[i],
                                                         0, 0, 0);
      }
    }
    bf16_t* row = act1 + (nt * 16 + lr) * 400 + g * 4;
    *reinterpret_cast<bf16x4*>(row + tile[0] * 16) =
        relu_bias_pack(acc[0], bias);
    if (two)
      *reinterpret_cast<bf16x4*>(row + tile[1] * 16) =
          relu_bias_pack(acc[1], bias);
  }
}

template <bool SAVE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void atari_encoder_fwd_kernel(
    const uint8_t* __restrict__ x,     // [N, 4, 84, 84]
    const bf16_t* __restrict__ w1,     // [32, 256]  c*64 + ky*8 + kx
    const float* __restrict__ b1,      // [32]
    const bf16_t* __restrict__ w2,     // [64, 512]  c*16 + ky*4 + kx
    const float* __restrict__ b2,      // [64]
    const bf16_t* __restrict__ w3,     // [64, 576]  c*9 + ky*3 + kx
    const float* __restrict__ b3,      // [64]
    bf16_t* __restrict__ out1,         // [N, 32, 20, 20] (SAVE only)
    bf16_t* __restrict__ out2,         // [N, 64, 9, 9]   (SAVE only)
    bf16_t* __restrict__ out3,         // [N, 64, 7, 7]
    long batch) {
  __shared__ __attribute__((aligned(16)))
  bf16_t lds[ENC_IMG_EL + ENC_ACT1_EL + ENC_OUT3_EL];
  bf16_t* const img = lds;                       // conv1 input row range
  bf16_t* const act2 = lds;                      // conv2 output (after conv1)
  bf16_t* const act1 = lds + ENC_IMG_EL;
  bf16_t* const o3 = lds + ENC_IMG_EL + ENC_ACT1_EL;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int g = lane >> 4, lr = lane & 15;

  // ---- weight fragments and biases of this wave's n-tiles, once ----------
  const int ch1 = (wave >> 1) * 16 + lr;         // conv1: 2 n-tiles, 2 waves each
  const int ch = wave * 16 + lr;                 // conv2/3: 4 n-tiles
  bf16x8 B1[8], B2[16], B3[18];
  #pragma unroll
  for (int kt = 0; kt < 8; ++kt)
    B1[kt] = *reinterpret_cast<const bf16x8*>(w1 + ch1 * 256 + kt * 32 + g * 8);
  #pragma unroll
  for (int kt = 0; kt < 16; ++kt)
    B2[kt] = *reinterpret_cast<const bf16x8*>(w2 + ch * 512 + kt * 32 + g * 8);
  // conv3 K order is tap*64 + c (act2 is channel-last): k-step kt covers tap
  // kt>>1, channels (kt&1)*32 + g*8 + j
  #pragma unroll
  for (int kt = 0; kt < 18; ++kt) {
    #pragma unroll
    for (int j = 0; j < 8; ++j)
      B3[kt][j] = w3[ch * 576 + ((kt & 1) * 32 + g * 8 + j) * 9 + (kt >> 1)];
  }
  const float bias1 = b1[ch1], bias2 = b2[ch], bias3 = b3[ch];

  // ---- per-lane A bases (the same for every image) ------------------------
  int base2[6], base3[4];
  #pragma unroll
  for (int mt = 0; mt < 6; ++mt) {
    const int px = min(mt * 16 + lr, 80);        // padded rows: clamped read
    const int oy = px / 9, ox = px - oy * 9;
    // k0 = kt*32 + g*8: channel kt*2 + (g>>1), window rows (g&1)*2, +1
    base2[mt] = (g >> 1) * 400 + (oy * 2 + (g & 1) * 2) * 20 + ox * 2;
  }
  #pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int px = min(mt * 16 + lr, 48);
    const int oy = px / 7, ox = px - oy * 7;
    base3[mt] = (oy * 9 + ox) * ENC_P3 + g * 8;
  }

  long n = blockIdx.x;
  uint4 pre[4];
  if (n < batch) load_half<0>(x + n * ENC_IMG_BYTES, pre, tid);

  for (; n < batch; n += gridDim.x) {
    const uint8_t* ximg = x + n * ENC_IMG_BYTES;

    // ---- conv1, rows 0..47 then 40..83 ------------------------------------
    store_half<0>(pre, img, tid);
    load_half<1>(ximg, pre, tid);
    __syncthreads();
    conv1_half<0>(img, act1, B1, bias1, wave, g, lr);
    __syncthreads();
    store_half<1>(pre, img, tid);
    __syncthreads();
    conv1_half<1>(img, act1, B1, bias1, wave, g, lr);
    __syncthreads();

    if (SAVE) {
      uint4* dst = reinterpret_cast<uint4*>(out1 + n * ENC_ACT1_EL);
      const uint4* src = reinterpret_cast<const uint4*>(act1);
      for (int i = tid; i < ENC_ACT1_EL / 8; i += 256) dst[i] = src[i];
    }

    // ---- conv2: act1 [32][20][20] -> act2 [81][72] -------------------------
    {
      f32x4 acc[6];
      #pragma unroll
      for (int mt = 0; mt < 6; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int kt = 0; kt < 16; ++kt) {
        #pragma unroll
        for (int mt = 0; mt < 6; ++mt) {
          const uint32_t* q = reinterpret_cast<const uint32_t*>(
              act1 + base2[mt] + kt * 800);
          const u32x4 v = {q[0], q[1], q[10], q[11]};  // 4 px of two rows
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              __builtin_bit_cast(bf16x8, v), B2[kt], acc[mt], 0, 0, 0);
        }
      }
      #pragma unroll
      for (int mt = 0; mt < 6; ++mt) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int px = mt * 16 + g * 4 + r;
          if (px < 81)
            act2[px * ENC_P3 + ch] = (bf16_t)fmaxf(acc[mt][r] + bias2, 0.f);
        }
      }
    }
    __syncthreads();

    if (SAVE) {
      // NCHW [64][81] from the channel-last plane, 8 elements per store
      uint4* dst = reinterpret_cast<uint4*>(out2 + n * (64 * 81));
      const uint16_t* src = reinterpret_cast<const uint16_t*>(act2);
      for (int v = tid; v < 64 * 81 / 8; v += 256) {
        int c = (v * 8) / 81, px = v * 8 - c * 81;
        uint32_t w[4];
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t e = src[px * ENC_P3 + c];
          w[j >> 1] = (j & 1) ? (w[j >> 1] | (e << 16)) : e;
          if (++px == 81) { px = 0; ++c; }
        }
        dst[v] = make_uint4(w[0], w[1], w[2], w[3]);
      }
    }

    // next image's first row range: in flight during conv3
    if (n + gridDim.x < batch)
      load_half<0>(x + (n + gridDim.x) * ENC_IMG_BYTES, pre, tid);

    // ---- conv3: act2 -> o3 [64][49] ----------------------------------------
    {
      f32x4 acc[4];
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int kt = 0; kt < 18; ++kt) {
        const int tap = kt >> 1;
        const int off = ((tap / 3) * 9 + tap % 3) * ENC_P3 + (kt & 1) * 32;
        #pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
          const bf16x8 a =
              *reinterpret_cast<const bf16x8*>(act2 + base3[mt] + off);
          acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, B3[kt], acc[mt],
                                                            0, 0, 0);
        }
      }
      #pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        #pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int px = mt * 16 + g * 4 + r;
          if (px < 49)
            o3[ch * 49 + px] = (bf16_t)fmaxf(acc[mt][r] + bias3, 0.f);
        }
      }
    }
    __syncthreads();

    {
      uint4* dst = reinterpret_cast<uint4*>(out3 + n * ENC_OUT3_EL);
      const uint4* src = reinterpret_cast<const uint4*>(o3);
      for (int i = tid; i < ENC_OUT3_EL / 8; i += 256) dst[i] = src[i];
    }
    // The next pass writes img (= act2) before its first barrier and act1
    // after it: act2's readers (conv3, the out2 copy) ended at the barrier
    // above, act1's (conv2, the out1 copy) at the one before.  o3 is written
    // again only after five more barriers.
  }
}

}  // namespace

// out1 and out2 are both given (training: backward needs them) or both null
// (inference).  No allocation, no synchronisation: safe under stream capture.
extern "C" int atari_encoder_fwd(const void* x, const void* w1,
                                 const float* b1, const void* w2,
                                 const float* b2, const void* w3,
                                 const float* b3, void* out1, void* out2,
                                 void* out3, long batch, hipStream_t stream) {
  if (batch <= 0) return 0;
  if ((out1 == nullptr) != (out2 == nullptr)) return (int)hipErrorInvalidValue;
  // CU count of the device of the first call, kept for all later calls:
  // the process's devices are taken to be alike (it only sizes the grid; any
  // grid >= 1 computes the same result).
  static int n_cu = 0;
  if (n_cu == 0) {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount,
                              dev) != hipSuccess || v <= 0)
      v = 256;
    n_cu = v;
  }
  const long resident = 2L * n_cu;               // two workgroups per CU
  const unsigned grid = (unsigned)(batch < resident ? batch : resident);
  if (out1) {
    hipLaunchKernelGGL(atari_encoder_fwd_kernel<true>, dim3(grid), dim3(256),
                       0, stream, (const uint8_t*)x, (const bf16_t*)w1, b1,
                       (const bf16_t*)w2, b2, (const bf16_t*)w3, b3,
                       (bf16_t*)out1, (bf16_t*)out2, (bf16_t*)out3, batch);
  } else {
    hipLaunchKernelGGL(atari_encoder_fwd_kernel<false>, dim3(grid), dim3(256),
                       0, stream, (const uint8_t*)x, (const bf16_t*)w1, b1,
                       (const bf16_t*)w2, b2, (const bf16_t*)w3, b3,
                       (bf16_t*)nullptr, (bf16_t*)nullptr, (bf16_t*)out3,
                       batch);
  }
  CHECK_LAUNCH();
  return 0;
}
