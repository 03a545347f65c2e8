// oc_policy_window.hip -- truncated windows for the recurrent learner (include/oc_policy.h, the section "windows
// of a rollout"): the snapshot that records the seat's state where a window begins, and the gather that packs a
// minibatch of windows into a sink-shaped batch of W slots and E envs, which the recurrent update then unrolls
// as it unrolls any sink.  Two plain copy kernels; a translation unit and code object of its own, between the
// seat's and the update's: the other units' kernels stay what they were.
//
// gfx950 only.  Neither kernel computes anything: every element is moved as the bits it is (4-byte rows as
// uint32, int8 rows as uint8, the timestep as uint64).
//
//   k_window_snapshot   a grid-stride copy of h and c, float [64][n] each, into the contiguous block
//                       states[slot / W] = [2][64][n]; 16-byte accesses where the three pointers allow (64 n is
//                       a multiple of 4), scalar otherwise.  Every workgroup reads *pos first and leaves at once
//                       unless slot % W == 0: at most 4 workgroups per CU are launched, so the W - 1 steps out of
//                       W on which nothing is copied cost an empty launch.
//   k_window_gather     thread = sequence e (grid-stride over x), y (grid-stride too) = slot t of the window (the F
//                       observation rows, then the eight per-sample rows) or, behind the W slots, the h or the
//                       c block's 64 rows.  e is the fastest index on both sides: with ids of 32 neighbouring
//                       envs of one window next to each other a wave reads two runs of 32 consecutive elements
//                       of every row and writes 64 consecutive ones.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/oc_policy.h"
#include "oc_policy_fail.h"

namespace {

using namespace ocpol;

constexpr int HID = OC_POLICY_HIDDEN;
constexpr int COPY_THREADS = 256;
constexpr unsigned SNAPSHOT_MAX_GROUPS = 1024;   // 4 per CU of a 256-CU part
constexpr unsigned GATHER_MAX_GROUPS_X = 4096, GATHER_MAX_GROUPS_Y = 1024;

// the sink's position word as every lane sees it (oc_rollout.hip's load_word / in_ring: the word was written
// by an earlier launch; a value outside 0 .. T - 1 is taken modulo T)
__device__ __forceinline__ long long load_pos(const long long *p, int T) {
  const long long v = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)v >> 32));
  long long s = (long long)(((unsigned long long)hi << 32) | lo);
  if ((unsigned long long)s >= (unsigned long long)T) {
    s %= T;
    if (s < 0) s += T;
  }
  return s;
}

struct SnapshotArgs {
  const long long *pos;
  const float *h, *c;
  float *states;
  int32_t T, W;
  uint32_t per;      // 64 n: the floats of h, and of c
  int32_t vec;       // h, c and states are 16-byte aligned
};

__global__ void __launch_bounds__(COPY_THREADS) k_window_snapshot(const SnapshotArgs a) {
  const long long slot = load_pos(a.pos, a.T);
  if (slot % a.W != 0) return;
  float *__restrict__ dst = a.states + (size_t)(slot / a.W) * 2u * a.per;   // [2][64][n]: h, then c
  const float *__restrict__ h = a.h;
  const float *__restrict__ c = a.c;
  const uint32_t stride = gridDim.x * COPY_THREADS, first = blockIdx.x * COPY_THREADS + threadIdx.x;
  const uint32_t per4 = a.vec ? a.per / 4 : 0;                             // float4s of each tensor
  for (uint32_t i = first; i < 2 * per4; i += stride)
    ((float4 *)dst)[i] = i < per4 ? ((const float4 *)h)[i] : ((const float4 *)c)[i - per4];
  for (uint32_t i = 4 * per4 + first; i < a.per; i += stride) {            // the scalar rest (all of it, unaligned)
    dst[i] = h[i];
    dst[a.per + i] = c[i];
  }
}

struct GatherArgs {
  oc_window_src src;
  oc_window_batch dst;
  const int32_t *seqs;
  uint32_t E;
};

template <typename T>
__device__ __forceinline__ void copy_rows(const T *__restrict__ src, T *__restrict__ dst, int rows, size_t n, size_t E) {
#pragma unroll 4
  for (int j = 0; j < rows; j++) dst[(size_t)j * E] = src[(size_t)j * n];
}

// OBS: the observation rows' element as bits (uint32_t: int32 and float32 rows; uint8_t: int8 rows)
template <typename OBS>
__global__ void __launch_bounds__(COPY_THREADS) k_window_gather(const GatherArgs a) {
  const oc_window_src &S = a.src;
  const oc_window_batch &D = a.dst;
  const size_t n = (size_t)S.n, E = a.E;
  const int W = S.W, F = S.F;
  for (int y = blockIdx.y; y < W + 2; y += gridDim.y)
  for (uint32_t e = blockIdx.x * COPY_THREADS + threadIdx.x; e < a.E; e += gridDim.x * COPY_THREADS) {
    const uint32_t s = (uint32_t)a.seqs[e];
    const size_t k = s / (uint32_t)n, env = s % (uint32_t)n;
    if (y < W) {                                       // slot t = y of the window: slot k W + t of the sink
      const size_t from = (k * W + y) * n + env, to = (size_t)y * E + e;
      copy_rows((const OBS *)S.obs + (k * W + y) * F * n + env, (OBS *)D.obs + (size_t)y * F * E + e, F, n, E);
      const uint64_t ts = ((const uint64_t *)S.timestep)[from];
      const uint32_t mv = ((const uint32_t *)S.actions)[2 * (k * W + y) * n + env];
      const uint32_t cm = ((const uint32_t *)S.actions)[(2 * (k * W + y) + 1) * n + env];
      const uint32_t lp = ((const uint32_t *)S.log_probs)[from], ad = ((const uint32_t *)S.advantages)[from];
      const uint32_t rt = ((const uint32_t *)S.returns)[from], es = ((const uint32_t *)S.episode_starts)[from];
      const uint32_t va = ((const uint32_t *)S.values)[from];
      ((uint64_t *)D.timestep)[to] = ts;
      ((uint32_t *)D.actions)[2 * (size_t)y * E + e] = mv;
      ((uint32_t *)D.actions)[(2 * (size_t)y + 1) * E + e] = cm;
      ((uint32_t *)D.log_probs)[to] = lp, ((uint32_t *)D.advantages)[to] = ad;
      ((uint32_t *)D.returns)[to] = rt, ((uint32_t *)D.episode_starts)[to] = es;
      ((uint32_t *)D.values)[to] = va;
    } else {                                           // states[k][y - W]: h (0) or c (1), 64 rows
      const int which = y - W;
      copy_rows((const uint32_t *)S.states + (2 * k + which) * HID * n + env,
                (uint32_t *)(which ? D.c0 : D.h0) + e, HID, n, E);
    }
  }
}

bool below_2_31(int64_t v) { return v < ((int64_t)1 << 31); }

int launched(const char *who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fail("%s: kernel launch: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace

extern "C" {

int oc_policy_window_snapshot(const int64_t *pos, int32_t T, int32_t W, const float *h, const float *c, float *states,
                              int64_t n, void *stream) {
  if (!pos || !h || !c || !states) return fail("oc_policy_window_snapshot: pos, h, c and states must not be NULL");
  if (W < 1 || T < 1 || T % W) return fail("oc_policy_window_snapshot: W >= 1 and T %% W == 0 (T %d, W %d)", T, W);
  if (n < 1) return fail("oc_policy_window_snapshot: n >= 1");
  if (!below_2_31((int64_t)HID * n)) return fail("oc_policy_window_snapshot: 64 n must stay below 2^31");
  SnapshotArgs a;
  memset(&a, 0, sizeof(a));
  a.pos = (const long long *)pos, a.h = h, a.c = c, a.states = states;
  a.T = T, a.W = W, a.per = (uint32_t)(HID * n);
  a.vec = (((uintptr_t)h | (uintptr_t)c | (uintptr_t)states) & 15) == 0;
  const uint32_t items = a.vec ? a.per / 2 : a.per;   // 2 * per / 4 float4s, or per scalar pairs
  unsigned groups = (items + COPY_THREADS - 1) / COPY_THREADS;
  if (groups > SNAPSHOT_MAX_GROUPS) groups = SNAPSHOT_MAX_GROUPS;
  hipLaunchKernelGGL(k_window_snapshot, dim3(groups), dim3(COPY_THREADS), 0, (hipStream_t)stream, a);
  return launched("oc_policy_window_snapshot");
}

int oc_policy_window_gather(const oc_window_src *src, const oc_window_batch *dst, const int32_t *seqs, int32_t E,
                            void *stream) {
  if (!src || !dst || !seqs) return fail("oc_policy_window_gather: src, dst and seqs must not be NULL");
  if (!src->obs || !src->timestep || !src->actions || !src->log_probs || !src->advantages || !src->returns ||
      !src->episode_starts || !src->values || !src->states)
    return fail("oc_policy_window_gather: a NULL pointer in src");
  if (!dst->obs || !dst->timestep || !dst->actions || !dst->log_probs || !dst->advantages || !dst->returns ||
      !dst->episode_starts || !dst->values || !dst->h0 || !dst->c0)
    return fail("oc_policy_window_gather: a NULL pointer in dst");
  if (src->W < 1 || src->T < 1 || src->T % src->W)
    return fail("oc_policy_window_gather: W >= 1 and T %% W == 0 (T %d, W %d)", src->T, src->W);
  if (E < 1) return fail("oc_policy_window_gather: E >= 1");
  if (src->n < 1) return fail("oc_policy_window_gather: n >= 1");
  if (src->F < 1 || src->F + 2 > 64) return fail("oc_policy_window_gather: F >= 1, F + 2 <= 64");
  if (src->obs_type < 0 || src->obs_type > 2) return fail("oc_policy_window_gather: obs_type 0..2");
  if (!below_2_31(HID * src->n)) return fail("oc_policy_window_gather: 64 n must stay below 2^31");
  if (!below_2_31((int64_t)src->T * src->n)) return fail("oc_policy_window_gather: T n must stay below 2^31");
  if (!below_2_31((int64_t)src->W * src->F * E)) return fail("oc_policy_window_gather: W F E must stay below 2^31");
  GatherArgs a;
  memset(&a, 0, sizeof(a));
  a.src = *src, a.dst = *dst, a.seqs = seqs, a.E = (uint32_t)E;
  unsigned gx = ((unsigned)E + COPY_THREADS - 1) / COPY_THREADS;
  if (gx > GATHER_MAX_GROUPS_X) gx = GATHER_MAX_GROUPS_X;
  unsigned gy = (unsigned)src->W + 2;
  if (gy > GATHER_MAX_GROUPS_Y) gy = GATHER_MAX_GROUPS_Y;
  const dim3 grid(gx, gy);
  if (src->obs_type == 1)
    hipLaunchKernelGGL(k_window_gather<uint8_t>, grid, dim3(COPY_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_window_gather<uint32_t>, grid, dim3(COPY_THREADS), 0, (hipStream_t)stream, a);
  return launched("oc_policy_window_gather");
}

}  // extern "C"
