// oc_hostio.hip -- liboc_hostio.so: one step's worth of the numpy API, packed for one PCIe copy
// (include/oc_hostio.h).  One lane = one env; the [F][n] rows are read coalesced, the [n][k]
// blocks are written with a stride (a few hundred KB per step: the launch count, not the
// bandwidth, is what this kernel removes -- ~17 torch launches per step before it).
//
// k_pack_host_tiled writes the same bytes for an `out` that lies across PCIe (host-mapped memory,
// oc_hostio_alloc): one workgroup = one tile of TILE envs, whose part of every [n][w] block and of
// every per-env vector is ONE contiguous span of `out`.  The tile's spans are laid out in LDS and
// stored 16 bytes per lane, consecutive lanes to consecutive addresses.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/oc_hostio.h"

namespace {

thread_local char g_err[256] = "";
int fail(const char *msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return -1;
}

struct Args {
  const void *obs;
  const int32_t *plan;
  const double *timestep, *reward, *ep_return;
  const int32_t *done, *ep_length;
  char *out;
  int64_t n;
  int32_t F, w64, w32, w8;
  int64_t off32, off_ts, off_rew, off_ret, off_done, off_len, off8;
};

template <int OT>
__global__ void __launch_bounds__(256) k_pack_host(const Args p) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  int64_t *b64 = (int64_t *)p.out + i * p.w64;
  float *b32 = (float *)(p.out + p.off32) + i * p.w32;
  int8_t *b8 = (int8_t *)(p.out + p.off8) + i * p.w8;
  for (int r = 0; r < p.F; r++) {
    const int e = p.plan[r];   // uniform
    const int64_t idx = (int64_t)r * p.n + i;
    int v;
    if (OT == 1) v = ((const int8_t *)p.obs)[idx];
    else if (OT == 2) v = (int)((const float *)p.obs)[idx];   // the rows hold integers
    else v = ((const int32_t *)p.obs)[idx];
    const int blk = e >> 16, col = e & 0xFFFF;
    if (blk == 0) b64[col] = v;
    else if (blk == 1) b32[col] = (float)v;
    else b8[col] = (int8_t)v;
  }
  ((float *)(p.out + p.off_ts))[i] = (float)p.timestep[i];
  if (p.reward) ((float *)(p.out + p.off_rew))[i] = (float)p.reward[i];
  if (p.ep_return) ((double *)(p.out + p.off_ret))[i] = p.ep_return[i];
  if (p.done) ((int32_t *)(p.out + p.off_done))[i] = p.done[i];
  if (p.ep_length) ((int32_t *)(p.out + p.off_len))[i] = p.ep_length[i];
}

void offsets(Args &a, bool rew, bool ret, bool done, bool len, int64_t &total) {
  int64_t o = a.n * a.w64 * 8;
  a.off_ret = o, o += ret ? a.n * 8 : 0;
  a.off32 = o, o += a.n * a.w32 * 4;
  a.off_ts = o, o += a.n * 4;
  a.off_rew = o, o += rew ? a.n * 4 : 0;
  a.off_done = o, o += done ? a.n * 4 : 0;
  a.off_len = o, o += len ? a.n * 4 : 0;
  a.off8 = o, o += a.n * a.w8;
  total = o;
}

// ---- the tiled form ---------------------------------------------------------------------------------
constexpr int TILE = 64;              // envs per workgroup (oc_pack_host_tile)
constexpr int TILED_THREADS = 256;
constexpr int TILED_LDS = 32768;      // bytes of span staging per workgroup
constexpr int SPANS = 8;              // blocks and per-env vectors of the layout
// every span starts at the next 16-byte line of LDS plus its global address modulo 16 (below)
constexpr int SPAN_SLACK = SPANS * 32;

struct TiledArgs {
  Args a;
  int32_t pass_envs;   // envs of a tile staged at once: TILE unless the blocks are too wide for the LDS
};

// One span: `bytes` bytes at global address g, staged at LDS offset `lds`, lds % 16 == g % 16.
struct Span {
  char *g;
  int32_t lds, bytes;
};

__device__ __forceinline__ Span place(char *out, int64_t off, int64_t env0, int envs, int env_bytes, int &cur) {
  Span s;
  s.g = out + off + env0 * env_bytes;
  s.bytes = envs * env_bytes;
  s.lds = ((cur + 15) & ~15) + (int)((uintptr_t)s.g & 15);
  cur = s.lds + s.bytes;
  return s;
}

// LDS -> global by threads t = 0 .. nt-1 of a group: the 16-byte lines of the span go out as one
// 16-byte store per lane; what lies in front of the first line and behind the last one (the span
// starts and ends on a multiple of ES only) goes out ES bytes at a time, at most 2 * (16 / ES - 1)
// stores, one lane each.
template <int ES>
__device__ __forceinline__ void store_span(const char *lds, const Span s, int t, int nt) {
  const int head = min(s.bytes, (int)(-(uintptr_t)s.g & 15));
  const int body = (s.bytes - head) & ~15;
  const char *src = lds + s.lds;
  for (int i = head + t * 16; i < head + body; i += nt * 16) *(uint4 *)(s.g + i) = *(const uint4 *)(src + i);
  const int nh = head / ES, ne = nh + (s.bytes - head - body) / ES;
  if (t < ne) {
    const int i = t < nh ? t * ES : head + body + (t - nh) * ES;
    if (ES == 8) *(uint64_t *)(s.g + i) = *(const uint64_t *)(src + i);
    else if (ES == 4) *(uint32_t *)(s.g + i) = *(const uint32_t *)(src + i);
    else s.g[i] = src[i];
  }
}

template <int OT>
__global__ void __launch_bounds__(TILED_THREADS) k_pack_host_tiled(const TiledArgs q) {
  __shared__ __attribute__((aligned(16))) char lds[TILED_LDS];
  const Args &p = q.a;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t tile0 = (int64_t)blockIdx.x * TILE;
  const int tile_envs = (int)min((int64_t)TILE, p.n - tile0);
  for (int e0 = 0; e0 < tile_envs; e0 += q.pass_envs) {
    const int E = min(q.pass_envs, tile_envs - e0);
    const int64_t env0 = tile0 + e0;
    int cur = 0;
    const Span s64 = place(p.out, 0, env0, E, p.w64 * 8, cur);
    const Span sret = place(p.out, p.off_ret, env0, p.ep_return ? E : 0, 8, cur);
    const Span s32 = place(p.out, p.off32, env0, E, p.w32 * 4, cur);
    const Span sts = place(p.out, p.off_ts, env0, E, 4, cur);
    const Span srew = place(p.out, p.off_rew, env0, p.reward ? E : 0, 4, cur);
    const Span sdone = place(p.out, p.off_done, env0, p.done ? E : 0, 4, cur);
    const Span slen = place(p.out, p.off_len, env0, p.ep_length ? E : 0, 4, cur);
    const Span s8 = place(p.out, p.off8, env0, E, p.w8, cur);
    if (e0) __syncthreads();      // the previous pass has been stored
    if (lane < E) {
      // the rows, one per wave at a time: 64 consecutive envs of a row per load instruction
      for (int r = wave; r < p.F; r += TILED_THREADS / 64) {
        const int e = p.plan[r];   // uniform
        const int64_t idx = (int64_t)r * p.n + env0 + lane;
        int v;
        if (OT == 1) v = ((const int8_t *)p.obs)[idx];
        else if (OT == 2) v = (int)((const float *)p.obs)[idx];   // the rows hold integers
        else v = ((const int32_t *)p.obs)[idx];
        const int blk = e >> 16, col = e & 0xFFFF;
        // lanes are w * (element size) bytes apart: bank conflicts on these writes (64-byte stride for
        // 8 int64 columns).  Left so: the span lies in LDS byte for byte as in `out`, which keeps the
        // store loop a straight copy; a padded row stride would need un-padding address arithmetic there.
        if (blk == 0) ((int64_t *)(lds + s64.lds))[lane * p.w64 + col] = v;
        else if (blk == 1) ((float *)(lds + s32.lds))[lane * p.w32 + col] = (float)v;
        else ((int8_t *)(lds + s8.lds))[lane * p.w8 + col] = (int8_t)v;
      }
      // the per-env vectors, one or two per wave
      const int64_t i = env0 + lane;
      if (wave == 0) ((float *)(lds + sts.lds))[lane] = (float)p.timestep[i];
      if (wave == 1 && p.reward) ((float *)(lds + srew.lds))[lane] = (float)p.reward[i];
      if (wave == 2 && p.done) ((int32_t *)(lds + sdone.lds))[lane] = p.done[i];
      if (wave == 3 && p.ep_length) ((int32_t *)(lds + slen.lds))[lane] = p.ep_length[i];
      if (wave == 0 && p.ep_return) ((double *)(lds + sret.lds))[lane] = p.ep_return[i];
    }
    __syncthreads();
    // the three blocks by the whole workgroup, the short vectors one wave each
    store_span<8>(lds, s64, t, TILED_THREADS);
    store_span<4>(lds, s32, t, TILED_THREADS);
    store_span<1>(lds, s8, t, TILED_THREADS);
    if (wave == 0) store_span<4>(lds, sts, lane, 64);
    if (wave == 1) store_span<4>(lds, srew, lane, 64);
    if (wave == 2) store_span<4>(lds, sdone, lane, 64);
    if (wave == 3) store_span<4>(lds, slen, lane, 64);
    if (wave == 1) store_span<8>(lds, sret, lane, 64);
  }
}

}  // namespace

extern "C" {

int oc_hostio_abi_version(void) { return OC_HOSTIO_ABI_VERSION; }
const char *oc_hostio_last_error(void) { return g_err; }

int64_t oc_pack_host_bytes(int32_t w64, int32_t w32, int32_t w8, int32_t has_reward, int32_t has_ep_return,
                           int32_t has_done, int32_t has_ep_length, int64_t n) {
  if (w64 < 0 || w32 < 0 || w8 < 0 || n < 0) return -1;
  Args a{};
  a.n = n, a.w64 = w64, a.w32 = w32, a.w8 = w8;
  int64_t total;
  offsets(a, has_reward, has_ep_return, has_done, has_ep_length, total);
  return total;
}

int oc_pack_host(const void *obs_rows, int32_t obs_type, int32_t F, const int32_t *plan, int32_t w64, int32_t w32,
                 int32_t w8, const double *timestep, const double *reward, const double *ep_return,
                 const int32_t *done, const int32_t *ep_length, void *out, int64_t n, void *stream) {
  if (!obs_rows || !plan || !timestep || !out || F < 1 || w64 < 0 || w32 < 0 || w8 < 0 || n < 0 || obs_type < 0 ||
      obs_type > 2)
    return fail("oc_pack_host: bad argument");
  if (n == 0) return 0;
  Args a{};
  a.obs = obs_rows, a.plan = plan, a.timestep = timestep, a.reward = reward, a.ep_return = ep_return;
  a.done = done, a.ep_length = ep_length, a.out = (char *)out, a.n = n, a.F = F;
  a.w64 = w64, a.w32 = w32, a.w8 = w8;
  int64_t total;
  offsets(a, reward != nullptr, ep_return != nullptr, done != nullptr, ep_length != nullptr, total);
  const int bs = 256;
  const int64_t grid = (n + bs - 1) / bs;
  if (grid > 0x7FFFFFFF) return fail("oc_pack_host: n too large");
  const dim3 g((unsigned)grid), b(bs);
  if (obs_type == 1) hipLaunchKernelGGL(k_pack_host<1>, g, b, 0, (hipStream_t)stream, a);
  else if (obs_type == 2) hipLaunchKernelGGL(k_pack_host<2>, g, b, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_pack_host<0>, g, b, 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "oc_pack_host: kernel launch: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

int oc_pack_host_tile(void) { return TILE; }

int oc_pack_host_tiled(const void *obs_rows, int32_t obs_type, int32_t F, const int32_t *plan, int32_t w64,
                       int32_t w32, int32_t w8, const double *timestep, const double *reward,
                       const double *ep_return, const int32_t *done, const int32_t *ep_length, void *out,
                       int64_t n, void *stream) {
  if (!obs_rows || !plan || !timestep || !out || F < 1 || w64 < 0 || w32 < 0 || w8 < 0 || n < 0 || obs_type < 0 ||
      obs_type > 2)
    return fail("oc_pack_host_tiled: bad argument");
  // whole spans are stored, so every column of every block has to be some row's (oc_hostio.h); the
  // plan is device memory: the sum is all that can be verified here
  if ((int64_t)w64 + w32 + w8 != F) return fail("oc_pack_host_tiled: w64 + w32 + w8 must equal F");
  const int64_t env_bytes = (int64_t)w64 * 8 + (int64_t)w32 * 4 + w8 + 8 + 4 * 4;
  if (env_bytes > TILED_LDS - SPAN_SLACK) return fail("oc_pack_host_tiled: blocks too wide (one env must fit the LDS)");
  if (n == 0) return 0;
  TiledArgs q{};
  Args &a = q.a;
  a.obs = obs_rows, a.plan = plan, a.timestep = timestep, a.reward = reward, a.ep_return = ep_return;
  a.done = done, a.ep_length = ep_length, a.out = (char *)out, a.n = n, a.F = F;
  a.w64 = w64, a.w32 = w32, a.w8 = w8;
  int64_t total;
  offsets(a, reward != nullptr, ep_return != nullptr, done != nullptr, ep_length != nullptr, total);
  const int64_t fit = (TILED_LDS - SPAN_SLACK) / env_bytes;
  q.pass_envs = (int32_t)(fit < TILE ? fit : TILE);
  const int64_t grid = (n + TILE - 1) / TILE;
  if (grid > 0x7FFFFFFF) return fail("oc_pack_host_tiled: n too large");
  const dim3 g((unsigned)grid), b(TILED_THREADS);
  if (obs_type == 1) hipLaunchKernelGGL(k_pack_host_tiled<1>, g, b, 0, (hipStream_t)stream, q);
  else if (obs_type == 2) hipLaunchKernelGGL(k_pack_host_tiled<2>, g, b, 0, (hipStream_t)stream, q);
  else hipLaunchKernelGGL(k_pack_host_tiled<0>, g, b, 0, (hipStream_t)stream, q);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "oc_pack_host_tiled: kernel launch: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

int oc_hostio_alloc(int64_t bytes, void **host, void **dev) {
  if (bytes <= 0 || !host || !dev) return fail("oc_hostio_alloc: bad argument");
  *host = *dev = nullptr;
  void *h = nullptr, *d = nullptr;
  hipError_t e = hipHostMalloc(&h, (size_t)bytes, hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "oc_hostio_alloc: hipHostMalloc: %s", hipGetErrorString(e));
    return (int)e;
  }
  e = hipHostGetDevicePointer(&d, h, 0);
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "oc_hostio_alloc: hipHostGetDevicePointer: %s", hipGetErrorString(e));
    (void)hipHostFree(h);
    return (int)e;
  }
  *host = h, *dev = d;
  return 0;
}

int oc_hostio_free(void *host) {
  if (!host) return fail("oc_hostio_free: bad argument");
  const hipError_t e = hipHostFree(host);
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "oc_hostio_free: hipHostFree: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // extern "C"
