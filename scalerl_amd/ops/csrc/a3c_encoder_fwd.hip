// Fused A3C encoder forward: the four 3x3 stride-2 pad-1 convolutions (+bias,
// ELU) of one 42x42 image run back to back in one workgroup, with every
// intermediate in LDS.
//
//   x [N,C,42,42] f32 -> bf16 (RNE)
//     conv 3x3 s2 p1 +b1, ELU -> out1 [N,32,21,21]   (441 px, 28 m-tiles)
//     conv 3x3 s2 p1 +b2, ELU -> out2 [N,32,11,11]   (121 px,  8 m-tiles)
//     conv 3x3 s2 p1 +b3, ELU -> out3 [N,32, 6, 6]   ( 36 px,  3 m-tiles)
//     conv 3x3 s2 p1 +b4, ELU -> out4 [N,32, 3, 3]   (  9 px,  1 m-tile)
//
// fp32 accumulation, bias and ELU (v > 0 ? v : expm1f(v)); each layer's result
// is rounded once to bf16.  HBM traffic per image is the C*7 KB frame in and
// 576 B of out4 out; the SAVE variant also streams out1..out3 for backward.
//
// Structure:
//  - persistent workgroups (2 per CU, 4 waves each) stride over the images.
//    Wave w owns n-tile w & 1 (16 of the 32 output channels) and loads that
//    tile's weight (B) fragments for all four layers ONCE, into registers,
//    before the image loop: <= 2 + 27 fragments = 116 VGPRs.  The two waves
//    of an n-tile (w >> 1 = 0, 1) take alternate m-tiles.
//  - act1..act3 are channel-last LDS planes with a zero halo: one cell of 40
//    bf16 (32 channels + 8 pad = 80 B) per pixel of the (S+2)x(S+2) padded
//    map, so padding costs no branch in the MFMA loops.  K order of layers
//    2..4 is tap*32 + c: one K-step is one filter tap, and a lane's A
//    fragment is one 16-byte LDS read (8 channels of one input pixel).  The B
//    fragments are gathered from the [32, c*9 + tap] weights to match, once.
//  - columns of a plane row are split by parity (even x first, then odd x).
//    A stride-2 convolution reads, for neighbouring output pixels, input
//    pixels two columns apart; after the split those are neighbouring cells,
//    80 B apart, and 8 consecutive lanes' 16-byte reads fall in 8 different
//    16-byte bank groups.  (With 16-byte aligned cells laid out in x order
//    the two-pixel stride is a multiple of 32 B, which cannot be.)
//  - conv1 (K = 9*C, zero-padded to 32, or 64 for C = 4) reads the frame from
//    a linear bf16 [C][42][42] LDS copy with a gathered A fragment: per lane
//    8 element offsets per K-step, fixed before the image loop, and three bit
//    masks (tap in row 0 / column 0 of the filter, k >= 9*C) that turn the
//    top/left padding and the K tail into zeros.  42 -> 21 never reaches the
//    bottom/right padding.  The next image's frame is loaded (16-byte global
//    loads) into registers while conv2..conv4 run.
//  - epilogue: C/D map gives channel = lane & 15, so one bias per lane; bias,
//    ELU and the bf16 rounding happen in registers and the value goes into
//    the next plane's interior (never the halo) and, in the SAVE variant and
//    for out4, to HBM in NCHW.
//  - the thin layers: conv3's 3 m-tiles go 2 + 1 to the two waves of an
//    n-tile, conv4's single m-tile keeps waves 0 and 1 busy while waves 2 and
//    3 already stage the next frame; the second resident workgroup of the CU
//    fills those gaps.
//  - LDS: act1 23*24 cells = 44160 B, frame / act2 13*14 cells = 14560 B
//    (the frame, <= 14112 B, is dead once conv1 is done; act2's halo cells
//    are cleared again for every image because the frame overwrote them),
//    act3 8*8 cells = 5120 B: 63840 B static, two workgroups per CU.
//    Four barriers per image.
//
// Fragment maps for v_mfma_f32_16x16x32_bf16: mfma.h.

#include "common.h"
#include "mfma.h"

namespace {

constexpr int A3C_PITCH = 40;        // bf16 per cell: 32 channels + 8 pad
constexpr int A3C_FRAME = 42 * 42;   // 1764 px = 441 * 4

// The haloed, parity-split plane of an SxS feature map.
template <int S>
struct Plane {
  static constexpr int HALO = S + 2;
  static constexpr int HALF = (HALO + 1) / 2;   // cells per parity of a row
  static constexpr int CELLS = HALO * 2 * HALF;
  static constexpr int EL = CELLS * A3C_PITCH;
  // cell of halo coordinates (y, x), 0 <= y, x < HALO
  __device__ static constexpr int cell(int y, int x) {
    return (y * 2 + (x & 1)) * HALF + (x >> 1);
  }
};

constexpr int A3C_R1_EL = Plane<11>::EL;        // frame / act2 region
constexpr int A3C_LDS_EL = Plane<21>::EL + A3C_R1_EL + Plane<6>::EL;
static_assert(4 * A3C_FRAME <= A3C_R1_EL, "the frame aliases act2");
static_assert(Plane<21>::EL % 8 == 0 && A3C_R1_EL % 8 == 0 &&
              A3C_LDS_EL % 8 == 0, "16-byte plane starts");
static_assert(A3C_LDS_EL * 2 <= 65536, "static LDS cap");

__device__ __forceinline__ bf16_t elu_bias(float acc, float bias) {
  const float v = acc + bias;
  return (bf16_t)(v > 0.f ? v : expm1f(v));
}

// One of layers 2..4: src plane (SIxSI map) -> dst plane (SOxSO map) and/or
// out (this image's NCHW [32][SO*SO] in HBM).  A wave takes m-tiles
// half, half + 2, ... (TW of them); tiles past the last read a clamped pixel
// and are dropped at the store.
template <int SI, int SO, int TW, bool TO_LDS, bool TO_HBM>
__device__ __forceinline__ void conv_taps(const bf16_t* src, bf16_t* dst,
                                          bf16_t* __restrict__ out,
                                          const bf16x8 (&B)[9], float bias,
                                          int half, int g, int lr, int ch) {
  using PI = Plane<SI>;
  using PO = Plane<SO>;
  constexpr int NPX = SO * SO;
  constexpr int NT = (NPX + 15) / 16;
  static_assert(2 * TW >= NT, "two waves cover the m-tiles");
  static_assert(2 * (SO - 1) + 2 < PI::HALO, "taps stay inside the plane");
  if (half >= NT) return;                            // wave-uniform
  int abase[TW];
  #pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int px = min((half + 2 * i) * 16 + lr, NPX - 1);
    const int oy = px / SO, ox = px - oy * SO;
    // tap (ky, kx) reads halo pixel (2*oy + ky, 2*ox + kx)
    abase[i] = (oy * 4 * PI::HALF + ox) * A3C_PITCH + g * 8;
  }
  f32x4 acc[TW];
  #pragma unroll
  for (int i = 0; i < TW; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  #pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap % 3;
    const int off = ((ky * 2 + (kx & 1)) * PI::HALF + (kx >> 1)) * A3C_PITCH;
    #pragma unroll
    for (int i = 0; i < TW; ++i) {
      const bf16x8 a = *reinterpret_cast<const bf16x8*>(src + abase[i] + off);
      acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, B[tap], acc[i],
                                                       0, 0, 0);
    }
  }
  #pragma unroll
  for (int i = 0; i < TW; ++i) {
    #pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int px = (half + 2 * i) * 16 + g * 4 + r;
      if (px < NPX) {
        const bf16_t v = elu_bias(acc[i][r], bias);
        if (TO_LDS) {
          const int y = px / SO, xx = px - y * SO;
          dst[PO::cell(y + 1, xx + 1) * A3C_PITCH + ch] = v;
        }
        if (TO_HBM) out[ch * NPX + px] = v;
      }
    }
  }
}

template <int C, bool SAVE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2)))
void a3c_encoder_fwd_kernel(
    const float* __restrict__ x,       // [N, C, 42, 42]
    const bf16_t* __restrict__ w1,     // [32, C*9]  c*9 + ky*3 + kx
    const float* __restrict__ b1,      // [32]
    const bf16_t* __restrict__ w2,     // [32, 288]  c*9 + ky*3 + kx
    const float* __restrict__ b2,
    const bf16_t* __restrict__ w3,
    const float* __restrict__ b3,
    const bf16_t* __restrict__ w4,
    const float* __restrict__ b4,
    bf16_t* __restrict__ out1,         // [N, 32, 21, 21] (SAVE only)
    bf16_t* __restrict__ out2,         // [N, 32, 11, 11] (SAVE only)
    bf16_t* __restrict__ out3,         // [N, 32, 6, 6]   (SAVE only)
    bf16_t* __restrict__ out4,         // [N, 32, 3, 3]
    long batch) {
  constexpr int K1 = 9 * C;
  constexpr int KS = (K1 + 31) / 32;             // conv1 K-steps: 1, or 2
  constexpr int VEC = C * A3C_FRAME / 4;         // float4 per frame
  constexpr int NV = (VEC + 255) / 256;          // ... per thread
  using P1 = Plane<21>;

  __shared__ __attribute__((aligned(16))) bf16_t lds[A3C_LDS_EL];
  bf16_t* const act1 = lds;
  bf16_t* const frame = lds + P1::EL;            // bf16 [C][42][42], linear
  bf16_t* const act2 = frame;                    // after conv1
  bf16_t* const act3 = frame + A3C_R1_EL;

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & (WAVE - 1);
  const int g = lane >> 4, lr = lane & 15;
  const int half = wave >> 1;                    // which m-tiles
  const int ch = (wave & 1) * 16 + lr;           // this lane's output channel

  // ---- weight fragments and biases of this wave's n-tile, once ------------
  bf16x8 B1[KS], B2[9], B3[9], B4[9];
  // conv1's gather, per K-step s and element j (k = s*32 + g*8 + j): the
  // frame offset of tap k relative to pixel (2*oy, 2*ox), and bit s*8 + j of
  // ky0 / kx0 / dead set where the tap is in filter row 0 / column 0 / k is
  // past the real K
  int koff[KS][8];
  unsigned ky0 = 0, kx0 = 0, dead = 0;
  #pragma unroll
  for (int s = 0; s < KS; ++s) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int k = s * 32 + g * 8 + j;
      const bool real = k < K1;
      B1[s][j] = real ? w1[ch * K1 + k] : (bf16_t)0.f;
      const int c = k / 9, tap = k - c * 9;
      const int ky = tap / 3, kx = tap - ky * 3;
      koff[s][j] = c * A3C_FRAME + (ky - 1) * 42 + kx - 1;
      const unsigned bit = 1u << (s * 8 + j);
      if (!real) dead |= bit;
      if (ky == 0) ky0 |= bit;
      if (kx == 0) kx0 |= bit;
    }
  }
  // One layer's 72 two-byte loads at a time: the fences keep the scheduler
  // from issuing all 216 before the first is packed, which spills.
  const int wbase = ch * 288 + g * 72;
  __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) B2[tap][j] = w2[wbase + j * 9 + tap];
  }
  __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) B3[tap][j] = w3[wbase + j * 9 + tap];
  }
  __builtin_amdgcn_sched_barrier(0);
  #pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    #pragma unroll
    for (int j = 0; j < 8; ++j) B4[tap][j] = w4[wbase + j * 9 + tap];
  }
  __builtin_amdgcn_sched_barrier(0);
  const float bias1 = b1[ch], bias2 = b2[ch], bias3 = b3[ch], bias4 = b4[ch];

  // ---- every plane zero once: the halos of act1 and act3 stay zero ---------
  for (int i = tid; i < A3C_LDS_EL / 8; i += 256)
    reinterpret_cast<uint4*>(lds)[i] = make_uint4(0u, 0u, 0u, 0u);

  long n = blockIdx.x;
  float4 pre[NV];
  if (n < batch) {
    const float4* src = reinterpret_cast<const float4*>(x + n * (C * A3C_FRAME));
    #pragma unroll
    for (int i = 0; i < NV; ++i)
      if (tid + i * 256 < VEC) pre[i] = src[tid + i * 256];
  }
  __syncthreads();

  for (; n < batch; n += gridDim.x) {
    // ---- frame -> bf16, linear ---------------------------------------------
    #pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int v = tid + i * 256;
      if (v < VEC) {
        const bf16x4 q = {(bf16_t)pre[i].x, (bf16_t)pre[i].y,
                          (bf16_t)pre[i].z, (bf16_t)pre[i].w};
        *reinterpret_cast<bf16x4*>(frame + v * 4) = q;
      }
    }
    __syncthreads();

    // ---- conv1: frame -> act1, 14 m-tiles per wave --------------------------
    #pragma unroll 2
    for (int i = 0; i < 14; ++i) {
      const int mt = half + 2 * i;
      const int px = min(mt * 16 + lr, 440);       // padded rows: clamped read
      const int oy = px / 21, ox = px - oy * 21;
      const int base = oy * 84 + ox * 2;
      const unsigned bad = dead | (oy == 0 ? ky0 : 0u) | (ox == 0 ? kx0 : 0u);
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
      #pragma unroll
      for (int s = 0; s < KS; ++s) {
        bf16x8 a;
        #pragma unroll
        for (int j = 0; j < 8; ++j) {
          const bool zero = (bad >> (s * 8 + j)) & 1u;
          const bf16_t e = frame[zero ? 0 : base + koff[s][j]];
          a[j] = zero ? (bf16_t)0.f : e;
        }
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, B1[s], acc, 0, 0, 0);
      }
      #pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int p = mt * 16 + g * 4 + r;
        if (p < 441) {
          const bf16_t v = elu_bias(acc[r], bias1);
          const int y = p / 21, xx = p - y * 21;
          act1[P1::cell(y + 1, xx + 1) * A3C_PITCH + ch] = v;
          if (SAVE) out1[(n * 32 + ch) * 441 + p] = v;
        }
      }
    }
    __syncthreads();

    // next image's frame: in flight during conv2..conv4
    if (n + gridDim.x < batch) {
      const float4* src = reinterpret_cast<const float4*>(
          x + (n + gridDim.x) * (C * A3C_FRAME));
      #pragma unroll
      for (int i = 0; i < NV; ++i)
        if (tid + i * 256 < VEC) pre[i] = src[tid + i * 256];
    }

    // act2's halo (and the unused 14th cell of its odd half rows), which the
    // frame overwrote; conv2 below writes interior cells only
    if (tid < Plane<11>::CELLS) {
      const int y = tid / 14, rem = tid - y * 14;
      const int xx = rem < 7 ? 2 * rem : 2 * (rem - 7) + 1;
      if (y == 0 || y == 12 || xx == 0 || xx >= 12) {
        uint4* cell = reinterpret_cast<uint4*>(act2 + tid * A3C_PITCH);
        #pragma unroll
        for (int q = 0; q < A3C_PITCH / 8; ++q)
          cell[q] = make_uint4(0u, 0u, 0u, 0u);
      }
    }

    conv_taps<21, 11, 4, true, SAVE>(act1, act2, out2 + n * (32 * 121), B2,
                                     bias2, half, g, lr, ch);
    __syncthreads();
    conv_taps<11, 6, 2, true, SAVE>(act2, act3, out3 + n * (32 * 36), B3,
                                    bias3, half, g, lr, ch);
    __syncthreads();
    conv_taps<6, 3, 1, false, true>(act3, nullptr, out4 + n * (32 * 9), B4,
                                    bias4, half, g, lr, ch);
    // The next pass writes the frame (= act2) before its first barrier: act2's
    // reader, conv3, ended at the barrier above.  act1 is written after that
    // first barrier (its reader conv2 ended two barriers ago) and act3 after
    // three more (its reader conv4 ends before the first).
  }
}

template <int C>
int launch_c(unsigned grid, hipStream_t stream, const float* x,
             const bf16_t* w1, const float* b1, const bf16_t* w2,
             const float* b2, const bf16_t* w3, const float* b3,
             const bf16_t* w4, const float* b4, bf16_t* out1, bf16_t* out2,
             bf16_t* out3, bf16_t* out4, long batch) {
  if (out1) {
    hipLaunchKernelGGL((a3c_encoder_fwd_kernel<C, true>), dim3(grid),
                       dim3(256), 0, stream, x, w1, b1, w2, b2, w3, b3, w4, b4,
                       out1, out2, out3, out4, batch);
  } else {
    hipLaunchKernelGGL((a3c_encoder_fwd_kernel<C, false>), dim3(grid),
                       dim3(256), 0, stream, x, w1, b1, w2, b2, w3, b3, w4, b4,
                       (bf16_t*)nullptr, (bf16_t*)nullptr, (bf16_t*)nullptr,
                       out4, batch);
  }
  CHECK_LAUNCH();
  return 0;
}

}  // namespace

// out1..out3 are all given (training: backward needs them) or all null
// (inference).  C outside 1..4 is code -5.  No allocation, no
// synchronisation: safe under stream capture.
extern "C" int a3c_encoder_fwd(const float* x, const void* w1, const float* b1,
                               const void* w2, const float* b2, const void* w3,
                               const float* b3, const void* w4,
                               const float* b4, void* out1, void* out2,
                               void* out3, void* out4, long batch, int channels,
                               hipStream_t stream) {
  if (channels < 1 || channels > 4) return -5;
  if (batch <= 0) return 0;
  if ((out1 == nullptr) != (out2 == nullptr) ||
      (out1 == nullptr) != (out3 == nullptr))
    return (int)hipErrorInvalidValue;
  // CU count of the device of the first call, kept for all later calls (it
  // only sizes the grid; any grid >= 1 computes the same result).
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
#define A3C_ENC_ARGS                                                          \
  grid, stream, x, (const bf16_t*)w1, b1, (const bf16_t*)w2, b2,             \
      (const bf16_t*)w3, b3, (const bf16_t*)w4, b4, (bf16_t*)out1,           \
      (bf16_t*)out2, (bf16_t*)out3, (bf16_t*)out4, batch
  switch (channels) {
    case 1: return launch_c<1>(A3C_ENC_ARGS);
    case 2: return launch_c<2>(A3C_ENC_ARGS);
    case 3: return launch_c<3>(A3C_ENC_ARGS);
    default: return launch_c<4>(A3C_ENC_ARGS);
  }
#undef A3C_ENC_ARGS
}
