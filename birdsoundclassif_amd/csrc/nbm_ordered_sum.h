// The ordered reduction behind every deterministic twin: the twin's workgroups STORE their partial results into
// slots of a workspace, and this kernel adds the slots in ascending slot order, one thread per output element -- no atomic,
// a fixed summation order, and every slot element that is read has been written by the launch before it (the workspace
// needs no zeroing).
//   out[grp][r][c] (+)= sum_{s = 0 .. slots-1} part[s * slot_stride + grp * part_gs + r * part_ld + c]     r < rows, c < cols
// TI: float or double partials; the sum is carried in TI and rounded once to TO.
#pragma once
#include "nbm_common.h"

namespace {

struct OrderedSumShape {
  int slots, groups, cols, accumulate;
  long long slot_stride, part_gs, part_ld, rows, out_gs, out_ld;
};

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void nbm_ordered_sum_kernel(const TI* __restrict__ part, TO* __restrict__ out,
                                                              const OrderedSumShape s) {
  const long long per_group = s.rows * s.cols, total = per_group * s.groups;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long grp = i / per_group, e = i - grp * per_group;
    const long long r = e / s.cols;
    const int c = (int)(e - r * s.cols);
    const TI* src = part + grp * s.part_gs + r * s.part_ld + c;
    TI acc = (TI)0;
    for (int k = 0; k < s.slots; ++k) acc += src[(long long)k * s.slot_stride];
    TO* dst = out + grp * s.out_gs + r * s.out_ld + c;
    *dst = s.accumulate ? (TO)(*dst + (TO)acc) : (TO)acc;
  }
}

// The same reduction for MANY slots and FEW outputs (bias gradients, BatchNorm statistics, the clip norm: hundreds to thousands of slots
// for a few hundred outputs, where one thread per output is a serial chain of dependent loads): one WAVE per output element.  Lane l adds
// the slots l, l + 64, l + 128, ... in ascending order, then the 64 lane sums are added by a fixed butterfly.  The order is a function of
// (slots) alone, so the result is as reproducible as the serial form's; which form runs is decided by the launch geometry only.
template <typename TI, typename TO>
__global__ __launch_bounds__(256) void nbm_ordered_sum_wave_kernel(const TI* __restrict__ part, TO* __restrict__ out,
                                                                   const OrderedSumShape s) {
  const long long per_group = s.rows * s.cols, total = per_group * s.groups;
  const int lane = threadIdx.x & 63;
  for (long long i = blockIdx.x * 4ll + (threadIdx.x >> 6); i < total; i += (long long)gridDim.x * 4) {
    const long long grp = i / per_group, e = i - grp * per_group;
    const long long r = e / s.cols;
    const int c = (int)(e - r * s.cols);
    const TI* src = part + grp * s.part_gs + r * s.part_ld + c;
    TI acc = (TI)0;
    for (int k = lane; k < s.slots; k += 64) acc += src[(long long)k * s.slot_stride];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
      TO* dst = out + grp * s.out_gs + r * s.out_ld + c;
      *dst = s.accumulate ? (TO)(*dst + (TO)acc) : (TO)acc;
    }
  }
}
constexpr int NBM_ORDERED_SUM_WAVE_SLOTS = 128;            // from this many slots on ...
constexpr long long NBM_ORDERED_SUM_WAVE_OUTPUTS = 1 << 16; // ... and up to this many outputs: one wave per output

template <typename TI, typename TO>
inline void nbm_ordered_sum_launch(const TI* part, TO* out, const OrderedSumShape& s, hipStream_t st) {
  const long long total = s.rows * s.cols * s.groups;
  if (s.slots >= NBM_ORDERED_SUM_WAVE_SLOTS && total <= NBM_ORDERED_SUM_WAVE_OUTPUTS) {
    const long long wg = (total + 3) / 4;
    hipLaunchKernelGGL((nbm_ordered_sum_wave_kernel<TI, TO>), dim3((unsigned)(wg < 1 ? 1 : wg)), dim3(256), 0, st, part, out, s);
    return;
  }
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL((nbm_ordered_sum_kernel<TI, TO>), dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(256), 0, st, part, out, s);
}

// the flat case: out[i] (+)= sum_s part[s * n + i]
template <typename TI, typename TO>
inline void nbm_ordered_sum_flat(const TI* part, int slots, long long n, TO* out, int accumulate, hipStream_t st) {
  OrderedSumShape s{};
  s.slots = slots; s.groups = 1; s.cols = 1; s.accumulate = accumulate;
  s.slot_stride = n; s.part_gs = 0; s.part_ld = 1; s.rows = n; s.out_gs = 0; s.out_ld = 1;
  nbm_ordered_sum_launch(part, out, s, st);
}

// Deterministic form of the bias-gradient flush of the Winograd / cell transform kernels (winograd.hip, cellwino.hip).  There thread t of
// workgroup w keeps the sums of channel chunk (w * 256 + t) % nvec (V floats each) over its grid-stride loop (the stride is a multiple of
// nvec).  Instead of LDS atomics followed by global ones, the per-thread sums go to LDS, one thread per channel adds the shares of its
// chunk in ascending thread order, and stores the result into the workgroup's own slot part[w][nvec * V]; nbm_ordered_sum adds the slots.
// Workgroup-uniform call (one barrier).
constexpr int NBM_BIAS_SLOTS_MAX = 8192 + 1024;      // the transforms' grids: <= 8192 workgroups, then up to a multiple of nvec <= 1024
template <int V>
__device__ __forceinline__ void nbm_bias_slot_store(const float (&bsum)[V], int nvec, float* __restrict__ part) {
  __shared__ float stage[256 * V];
#pragma unroll
  for (int e = 0; e < V; ++e) stage[threadIdx.x * V + e] = bsum[e];
  __syncthreads();
  const int base = (int)((blockIdx.x * 256u) % (unsigned)nvec);
  float* slot = part + (long long)blockIdx.x * nvec * V;
  for (int k = threadIdx.x; k < nvec * V; k += 256) {
    const int c = k / V, e = k - c * V;
    float s = 0.f;
    for (int t = (c + nvec - base) % nvec; t < 256; t += nvec) s += stage[t * V + e];
    slot[k] = s;
  }
}
// host side: workgroups x N floats behind `workspace`, then the ordered sum into bias_grad (+=, like the atomics it replaces)
inline bool nbm_bias_slots_fit(const void* workspace, long long workspace_bytes, long long blocks, int N) {
  return workspace && workspace_bytes >= blocks * N * 4;
}

}  // namespace
