// Wav payload decoder: the interleaved sample bytes of a RIFF/WAVE `data` chunk -> mono float32 rows, bit for bit what
// prepare_dataset.read_wav (= librosa.load(sr=None, mono=True) of the reference, prepare_dataset.py:162) makes of the same
// bytes on the host.  A streaming kernel: every byte is read once with aligned 16-byte loads, every float is stored once.
//
// Per-channel value (float32):  PCM 8 (unsigned) (u8 - 128) / 128,  PCM 16 / 24  i / 2^(bits-1)  (all exact),  PCM 32
// (float)i32 (nearest even) * 2^-31 (= the float64 quotient rounded once),  float 32 the bits themselves,  float 64 rounded
// to nearest even.  Down-mix = numpy's `y.mean(1, dtype=float32)`: float32 sum left to right for 2 .. 7 channels, numpy's
// pairwise order ((c0+c1)+(c2+c3))+((c4+c5)+(c6+c7)) for 8, then ONE correctly rounded division by the channel count.  One
// channel is copied without arithmetic, so NaN payloads of a float file survive.  This file is compiled with
// -ffp-contract=off (Makefile): nothing here may be fused.
#include <utility>
#include "nbm_common.h"

namespace {

constexpr int TPB = 256;
enum { WAV_U8 = 0, WAV_I16, WAV_I24, WAV_I32, WAV_F32, WAV_F64, WAV_FORMATS };

constexpr int wav_sample_bytes(int fmt) {
  return fmt == WAV_U8 ? 1 : fmt == WAV_I16 ? 2 : fmt == WAV_I24 ? 3 : fmt == WAV_F64 ? 8 : 4;
}
// Frames per lane: the smallest multiple of 4 (float4 stores) whose bytes are a multiple of 16 (dwordx4 loads), so that a
// lane's span starts and ends on a 16-byte boundary of a 16-byte aligned row whatever the frame size (3, 6, 9, 21 ... bytes).
constexpr int wav_span_frames(int frame_bytes) {
  int f = 4;
  while ((f * frame_bytes) % 16) f += 4;
  return f;
}

// Sample at the compile-time byte offset `o` of the words w[0 .. nw) (little endian), as float32.
template <int FMT>
__device__ __forceinline__ float wav_sample(const uint32_t* w, int nw, int o) {
  const int k = o >> 2, sh = 8 * (o & 3);
  const uint32_t lo = w[k];
  const uint32_t hi = k + 1 < nw ? w[k + 1] : 0u;
  if constexpr (FMT == WAV_U8) {
    return (float)((int)((lo >> sh) & 0xFFu) - 128) * (1.0f / 128.0f);
  } else if constexpr (FMT == WAV_I16) {
    return (float)(int16_t)(lo >> sh) * (1.0f / 32768.0f);
  } else if constexpr (FMT == WAV_I24) {
    const uint32_t v = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh);
    return (float)(((int32_t)(v << 8)) >> 8) * (1.0f / 8388608.0f);
  } else if constexpr (FMT == WAV_I32) {
    return (float)(int32_t)lo * (1.0f / 2147483648.0f);
  } else if constexpr (FMT == WAV_F32) {
    return __uint_as_float(lo);
  } else {
    return (float)__longlong_as_double((long long)((((uint64_t)hi) << 32) | lo));
  }
}

// numpy's float32 mean over the channel axis (see the head of the file).  s / CH through float64: the float64 quotient of two
// float32 values rounded to float32 is the correctly rounded float32 quotient (53 >= 2 * 24 + 2 bits), with no reliance on
// how the compiler expands a float32 division.
template <int CH>
__device__ __forceinline__ float wav_downmix(const float* c) {
  if constexpr (CH == 1) {
    return c[0];
  } else {
    float s;
    if constexpr (CH == 8) {
      s = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
    } else {
      s = c[0];
#pragma unroll
      for (int i = 1; i < CH; ++i) s = s + c[i];
    }
    if constexpr ((CH & (CH - 1)) == 0) return s * (1.0f / (float)CH);   // power of two: the product is the rounded quotient
    else return (float)((double)s / (double)CH);
  }
}

template <int FMT, int CH>
__global__ __launch_bounds__(TPB) void wav_decode_kernel(const uint8_t* __restrict__ in, long long in_pitch, long long n,
                                                         float* __restrict__ out, long long out_pitch, int vec_store) {
  constexpr int BPS = wav_sample_bytes(FMT), FB = BPS * CH;
  constexpr int F = wav_span_frames(FB), NV = F * FB / 16, NW = 4 * NV;
  const uint8_t* row = in + (long long)blockIdx.y * in_pitch;
  float* o = out + (long long)blockIdx.y * out_pitch;
  const long long spans = n / F;                                        // whole spans; the < F frames behind them: below
  for (long long s = blockIdx.x * (long long)blockDim.x + threadIdx.x; s < spans; s += (long long)gridDim.x * blockDim.x) {
    const uint4* p = reinterpret_cast<const uint4*>(row + s * (long long)(F * FB));
    uint32_t w[NW];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      const uint4 v = p[k];
      w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w;
    }
    float r[F];
#pragma unroll
    for (int f = 0; f < F; ++f) {
      float c[CH];
#pragma unroll
      for (int ch = 0; ch < CH; ++ch) c[ch] = wav_sample<FMT>(w, NW, (f * CH + ch) * BPS);
      r[f] = wav_downmix<CH>(c);
    }
    float* dst = o + s * F;
    if (vec_store) {
#pragma unroll
      for (int f = 0; f < F; f += 4) {
        const f32x4 v = {r[f], r[f + 1], r[f + 2], r[f + 3]};
        *reinterpret_cast<f32x4*>(dst + f) = v;
      }
    } else {                                                             // a row pitch that is not a multiple of 4 floats
#pragma unroll
      for (int f = 0; f < F; ++f) dst[f] = r[f];
    }
  }
  // ragged tail: fewer than F <= 16 frames per row, one lane each, read byte by byte so that nothing behind n * FB is touched
  const long long t = spans * F + threadIdx.x;
  if (blockIdx.x == 0 && t < n) {
    const uint8_t* q = row + t * FB;
    float c[CH];
#pragma unroll
    for (int ch = 0; ch < CH; ++ch) {
      uint32_t w[2] = {0u, 0u};
#pragma unroll
      for (int b = 0; b < BPS; ++b) w[b >> 2] |= (uint32_t)q[ch * BPS + b] << (8 * (b & 3));
      c[ch] = wav_sample<FMT>(w, 2, 0);
    }
    o[t] = wav_downmix<CH>(c);
  }
}

typedef void (*wav_kernel_t)(const uint8_t*, long long, long long, float*, long long, int);

template <int FMT, int... CH>
constexpr void wav_fill_row(wav_kernel_t* row, std::integer_sequence<int, CH...>) {
  ((row[CH] = wav_decode_kernel<FMT, CH + 1>), ...);
}

wav_kernel_t wav_kernel(int fmt, int channels) {
  static wav_kernel_t table[WAV_FORMATS][NBM_WAV_MAX_CHANNELS];
  static const bool filled = [] {
    using seq = std::make_integer_sequence<int, NBM_WAV_MAX_CHANNELS>;
    wav_fill_row<WAV_U8>(table[WAV_U8], seq{});
    wav_fill_row<WAV_I16>(table[WAV_I16], seq{});
    wav_fill_row<WAV_I24>(table[WAV_I24], seq{});
    wav_fill_row<WAV_I32>(table[WAV_I32], seq{});
    wav_fill_row<WAV_F32>(table[WAV_F32], seq{});
    wav_fill_row<WAV_F64>(table[WAV_F64], seq{});
    return true;
  }();
  (void)filled;
  return table[fmt][channels - 1];
}

}  // namespace

extern "C" int nbm_wav_decode(const void* raw, int64_t raw_pitch, int batch, int tag, int bits, int channels, int64_t n,
                              float* out, int64_t out_pitch, void* stream) {
  if (!raw || !out || batch <= 0 || batch > 65535 || n <= 0) return NBM_EINVAL;
  int fmt = -1;
  if (tag == 1) fmt = bits == 8 ? WAV_U8 : bits == 16 ? WAV_I16 : bits == 24 ? WAV_I24 : bits == 32 ? WAV_I32 : -1;
  else if (tag == 3) fmt = bits == 32 ? WAV_F32 : bits == 64 ? WAV_F64 : -1;
  if (fmt < 0 || channels < 1 || channels > NBM_WAV_MAX_CHANNELS) return NBM_EUNSUPPORTED;
  const int fb = wav_sample_bytes(fmt) * channels;
  if (n > INT64_MAX / fb || raw_pitch < n * fb || out_pitch < n) return NBM_EINVAL;
  if (!nbm_aligned16(raw) || (batch > 1 && (raw_pitch & 15))) return NBM_EALIGN;
  if (((uintptr_t)out) & 3u) return NBM_EALIGN;
  const int vec_store = nbm_aligned16(out) && (batch == 1 || (out_pitch & 3) == 0);
  const long long spans = n / wav_span_frames(fb);
  long long gx = (spans + TPB - 1) / TPB;
  const long long cap = batch >= 512 ? 8 : 4096 / batch;
  gx = gx < 1 ? 1 : (gx > cap ? cap : gx);
  hipLaunchKernelGGL(wav_kernel(fmt, channels), dim3((unsigned)gx, (unsigned)batch), dim3(TPB), 0, (hipStream_t)stream,
                     (const uint8_t*)raw, (long long)raw_pitch, (long long)n, out, (long long)out_pitch, vec_store);
  return nbm_launch_status();
}
