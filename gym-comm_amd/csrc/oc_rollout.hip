// oc_rollout.hip -- liboc_rollout.so: a learner's rollout buffer beside the env (include/oc_rollout.h).
// Recording a step (oc_rollout_add, oc_rollout_add_reward) and generalised advantage estimation
// over the recorded steps (oc_rollout_gae), ONE launch each, all driven by the buffer's device-side
// counters -- ~16 torch launches per recorded step and a Python loop over n_steps before it.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/oc_rollout.h"

namespace {

thread_local char g_err[256] = "";
int fail(const char *fn, const char *msg) {
  snprintf(g_err, sizeof(g_err), "%s: %s", fn, msg);
  return -1;
}

#define RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// a counter word as every lane of the wave sees it: a vector load that bypasses this CU's L1 (the
// word was written by an earlier launch's last workgroup), made wave-uniform; a value outside
// 0..T-1 is taken modulo T so that no slot address can leave the buffer
__device__ __forceinline__ long long load_word(const long long *p) {
  const long long v = __hip_atomic_load(p, RLX_AGENT);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ long long in_ring(long long p, int T) {
  if ((unsigned long long)p >= (unsigned long long)T) {
    p %= T;
    if (p < 0) p += T;
  }
  return p;
}

// ---- oc_rollout_add ---------------------------------------------------------------------------
// A slot is F + 7 row TASKS of n elements each: the F observation rows, then timestep (8 bytes per
// env), move, comm, log_prob, episode_start, value (4 bytes) and the reward row's zero (8 bytes, no
// source).  blockIdx.y picks `per_group` consecutive tasks, blockIdx.x (grid-stride) the envs; a wave
// loads up to eight rows, then stores them, each access 64 consecutive elements of one row.
enum { TASK_TS = 0, TASK_MOVE, TASK_COMM, TASK_LOGP, TASK_ES, TASK_VALUE, TASK_REWARD, TASK_EXTRA };

struct AddArgs {
  void *obs;
  double *timestep;
  int32_t *actions;
  float *log_probs, *values, *episode_starts;
  double *rewards;
  long long *pos, *last, *count;
  int *ticket;
  const void *rows;
  const double *ts;
  const int32_t *move, *comm;
  const float *log_prob, *value, *es;
  uint32_t n;
  int32_t T, F, per_group;
};

struct Slot {   // the slot's rows (64-bit bases; offsets inside a slot are 32-bit)
  double *timestep, *rewards;
  int32_t *actions;
  float *log_probs, *values, *episode_starts;
};

constexpr int ADD_AHEAD = 8;   // observation rows a lane has in flight before it stores the first

template <typename E>
__global__ void __launch_bounds__(256) k_rollout_add(const AddArgs a) {
  // every workgroup reads the position BEFORE its first store (the source loads below do not wait for
  // it); the count with it: both words are written by an EARLIER launch's last workgroup only
  const long long p = in_ring(load_word(a.pos), a.T);
  const long long c = load_word(a.count);
  const size_t row = (size_t)p * a.n;
  const E *src = (const E *)a.rows;
  E *dst = (E *)a.obs + row * (size_t)a.F;
  Slot s;
  s.timestep = a.timestep + row, s.rewards = a.rewards + row;
  s.actions = a.actions + 2 * row;
  s.log_probs = a.log_probs + row, s.values = a.values + row, s.episode_starts = a.episode_starts + row;
  const int t0 = (int)blockIdx.y * a.per_group;
  const int t1 = min(t0 + a.per_group, a.F + TASK_EXTRA);
  const int o1 = min(t1, a.F);                       // this group's observation rows: t0 .. o1 - 1
  const int x0 = t0 - a.F, x1 = t1 - a.F;            // ... and its extra tasks: those k with x0 <= k < x1
  const bool do_ts = x0 <= TASK_TS && TASK_TS < x1, do_move = x0 <= TASK_MOVE && TASK_MOVE < x1;
  const bool do_comm = x0 <= TASK_COMM && TASK_COMM < x1, do_logp = x0 <= TASK_LOGP && TASK_LOGP < x1;
  const bool do_es = x0 <= TASK_ES && TASK_ES < x1;
  const bool do_value = x0 <= TASK_VALUE && TASK_VALUE < x1 && a.value != nullptr;
  const bool do_reward = x0 <= TASK_REWARD && TASK_REWARD < x1;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < (int64_t)a.n; e += (int64_t)gridDim.x * 256) {
    const uint32_t i = (uint32_t)e;
    for (int t = t0; t < o1; t += ADD_AHEAD) {
      E v[ADD_AHEAD];
#pragma unroll
      for (int u = 0; u < ADD_AHEAD; u++)
        if (t + u < o1) v[u] = src[(uint32_t)(t + u) * a.n + i];
#pragma unroll
      for (int u = 0; u < ADD_AHEAD; u++)
        if (t + u < o1) dst[(uint32_t)(t + u) * a.n + i] = v[u];
    }
    if (x1 > 0) {                                    // all loads, then all stores
      double ts = 0.0;
      int32_t mv = 0, cm = 0;
      float lp = 0.f, es = 0.f, val = 0.f;
      if (do_ts) ts = a.ts[i];
      if (do_move) mv = a.move[i];
      if (do_comm) cm = a.comm[i];
      if (do_logp) lp = a.log_prob[i];
      if (do_es) es = a.es[i];
      if (do_value) val = a.value[i];
      if (do_ts) s.timestep[i] = ts;
      if (do_move) s.actions[i] = mv;
      if (do_comm) s.actions[a.n + i] = cm;
      if (do_logp) s.log_probs[i] = lp;
      if (do_es) s.episode_starts[i] = es;
      if (do_value) s.values[i] = val;
      if (do_reward) s.rewards[i] = 0.0;
    }
  }
  // The ticket.  Every storing wave drains its stores, the workgroup meets, ONE lane releases at agent
  // scope and draws; the workgroup that draws the last ticket knows every other one has read *pos and
  // finished, and alone moves the counters.  (The explicit wait after the release fence stays: the
  // compiler may drop the fence's own when it thinks the scoreboard empty.)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int total = (int)(gridDim.x * gridDim.y);
    const int drawn = __hip_atomic_fetch_add(a.ticket, 1, RLX_AGENT);
    if (drawn == total - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      __hip_atomic_store(a.last, p, RLX_AGENT);
      __hip_atomic_store(a.pos, p + 1 >= a.T ? 0 : p + 1, RLX_AGENT);
      __hip_atomic_store(a.count, c + 1, RLX_AGENT);
      __hip_atomic_store(a.ticket, 0, RLX_AGENT);
    }
  }
}

// ---- oc_rollout_add_reward --------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_rollout_add_reward(double *rewards, int32_t *dones, const long long *last,
                                                            const double *r, const int32_t *d, uint32_t n, int32_t T) {
  const long long p = in_ring(load_word(last), T);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n) return;
  const size_t at = (size_t)p * n + (size_t)i;
  rewards[at] = rewards[at] + r[i];
  dones[at] = d[i];
}

// ---- oc_rollout_gae ---------------------------------------------------------------------------
// One lane per env, newest step to oldest.  Only the `last` chain is serial: the rows of the NEXT
// eight steps are requested before the current eight are consumed (loads retire in issue order, so
// the wait for the current block leaves the next one in flight), and the stores never wait.
struct GaeArgs {
  const double *rewards;
  const float *values, *episode_starts;
  float *advantages, *returns;
  const long long *pos, *count;
  const float *last_values, *last_dones;
  uint32_t n;
  int32_t T;
  float g, gl;
};

constexpr int GAE_AHEAD = 8;

struct GaeBlock {
  double r[GAE_AHEAD];
  float v[GAE_AHEAD], e[GAE_AHEAD];
};

// steps at slots s, s-1, ... (wrapping), `m` of them
__device__ __forceinline__ void gae_load(const GaeArgs &a, GaeBlock &b, int s, int m, uint32_t i) {
#pragma unroll
  for (int u = 0; u < GAE_AHEAD; u++) {
    if (u < m) {
      int sl = s - u;
      if (sl < 0) sl += a.T;
      const size_t at = (size_t)sl * a.n + i;
      b.r[u] = a.rewards[at];
      b.v[u] = a.values[at];
      b.e[u] = a.episode_starts[at];
    }
  }
}

__global__ void __launch_bounds__(64) k_rollout_gae(const GaeArgs a) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (e >= (int64_t)a.n) return;
  const uint32_t i = (uint32_t)e;
  const long long pos = in_ring(load_word(a.pos), a.T);
  const long long cnt = load_word(a.count);
  int left = cnt < 0 ? 0 : (cnt > a.T ? a.T : (int)cnt);    // L
  if (left == 0) return;
  int s = pos == 0 ? a.T - 1 : (int)pos - 1;                // slot of the newest step
  float nv = a.last_values[i];
  float nnt = 1.0f - a.last_dones[i];
  float last = 0.0f;
  GaeBlock cur, nxt;
  gae_load(a, cur, s, min(left, GAE_AHEAD), i);
  while (left > 0) {
    const int m = min(left, GAE_AHEAD);
    int sn = s - m;
    if (sn < 0) sn += a.T;
    gae_load(a, nxt, sn, min(left - m, GAE_AHEAD), i);
#pragma unroll
    for (int u = 0; u < GAE_AHEAD; u++) {
      if (u < m) {
        int sl = s - u;
        if (sl < 0) sl += a.T;
        const size_t at = (size_t)sl * a.n + i;
        const float v = cur.v[u];
        const float delta = ((float)cur.r[u] + (a.g * nv) * nnt) - v;
        last = delta + ((a.gl * nnt) * last);
        a.advantages[at] = last;
        a.returns[at] = last + v;
        nv = v;
        nnt = 1.0f - cur.e[u];
      }
    }
    cur = nxt;
    s = sn;
    left -= m;
  }
}

// ---- host -------------------------------------------------------------------------------------
int launched(const char *fn) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_err, sizeof(g_err), "%s: kernel launch: %s", fn, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

int elem_size(int32_t obs_type) { return obs_type == 1 ? 1 : 4; }

// what every entry point checks, before any device call
int check_buf(const char *fn, const oc_rollout_buf *b) {
  if (!b) return fail(fn, "NULL buffer");
  if (b->n <= 0) return fail(fn, "n <= 0");
  if (b->T <= 0) return fail(fn, "T <= 0");
  if (b->F <= 0) return fail(fn, "F <= 0");
  if (b->obs_type < 0 || b->obs_type > 2) return fail(fn, "unknown obs_type");
  // offsets inside a slot are 32-bit
  if (b->n >= (1ll << 31) || (int64_t)b->F * b->n * elem_size(b->obs_type) >= (1ll << 31))
    return fail(fn, "a slot of 2 GiB or more");
  if (!b->obs || !b->timestep || !b->actions || !b->log_probs || !b->values || !b->episode_starts || !b->rewards ||
      !b->dones || !b->pos || !b->last || !b->count)
    return fail(fn, "NULL buffer tensor");
  return 0;
}

// oc_rollout_add's launch: gridDim.x workgroup columns over the env blocks, `groups` rows of
// `per_group` consecutive tasks each.
// Launch- and latency-bound at a few thousand envs: a lone wave storing all F + 7 rows back to back
// pays every store's issue in series, so the rows are dealt over ~512 workgroups (two per CU).  Never
// more: each workgroup ends in one add on ONE word, which serves ~88 of them per microsecond.
struct AddPlan {
  int32_t gx, groups, per_group;
};
AddPlan add_plan(const oc_rollout_buf *buf) {
  const int tasks = buf->F + TASK_EXTRA, target = 512;
  const int64_t env_blocks = (buf->n + 255) / 256;
  int groups = (int)((target + env_blocks - 1) / env_blocks);
  groups = groups < 1 ? 1 : (groups > tasks ? tasks : groups);
  const int per_group = (tasks + groups - 1) / groups;
  groups = (tasks + per_group - 1) / per_group;
  int64_t gx = target / groups;
  gx = gx < 1 ? 1 : (gx > env_blocks ? env_blocks : gx);
  return AddPlan{(int32_t)gx, groups, per_group};
}

}  // namespace

extern "C" {

int oc_rollout_abi_version(void) { return OC_ROLLOUT_ABI_VERSION; }
const char *oc_rollout_last_error(void) { return g_err; }

int oc_rollout_add(const oc_rollout_buf *buf, const void *rows, const double *timestep, const int32_t *move,
                   const int32_t *comm, const float *log_prob, const float *value, const float *episode_start,
                   void *stream) {
  static const char fn[] = "oc_rollout_add";
  if (const int rc = check_buf(fn, buf)) return rc;
  if (!buf->ticket) return fail(fn, "NULL ticket");
  if (!rows || !timestep || !move || !comm || !log_prob || !episode_start) return fail(fn, "NULL input row");
  AddArgs a{};
  a.obs = buf->obs, a.timestep = buf->timestep, a.actions = buf->actions, a.log_probs = buf->log_probs;
  a.values = buf->values, a.episode_starts = buf->episode_starts, a.rewards = buf->rewards;
  a.pos = (long long *)buf->pos, a.last = (long long *)buf->last, a.count = (long long *)buf->count;
  a.ticket = buf->ticket;
  a.rows = rows, a.ts = timestep, a.move = move, a.comm = comm, a.log_prob = log_prob, a.value = value;
  a.es = episode_start;
  a.n = (uint32_t)buf->n, a.T = buf->T, a.F = buf->F;
  const AddPlan plan = add_plan(buf);
  a.per_group = plan.per_group;
  const dim3 g((unsigned)plan.gx, (unsigned)plan.groups), b(256);
  if (buf->obs_type == 1) hipLaunchKernelGGL(k_rollout_add<int8_t>, g, b, 0, (hipStream_t)stream, a);
  else hipLaunchKernelGGL(k_rollout_add<int32_t>, g, b, 0, (hipStream_t)stream, a);   // float32 rows: the same bits
  return launched(fn);
}

int oc_rollout_add_plan(const oc_rollout_buf *buf, int32_t plan[3]) {
  static const char fn[] = "oc_rollout_add_plan";
  if (const int rc = check_buf(fn, buf)) return rc;
  if (!plan) return fail(fn, "NULL plan");
  const AddPlan p = add_plan(buf);
  plan[0] = p.gx, plan[1] = p.groups, plan[2] = p.per_group;
  return 0;
}

int oc_rollout_add_reward(const oc_rollout_buf *buf, const double *rewards, const int32_t *dones, void *stream) {
  static const char fn[] = "oc_rollout_add_reward";
  if (const int rc = check_buf(fn, buf)) return rc;
  if (!rewards || !dones) return fail(fn, "NULL input row");
  const dim3 g((unsigned)((buf->n + 255) / 256)), b(256);
  hipLaunchKernelGGL(k_rollout_add_reward, g, b, 0, (hipStream_t)stream, buf->rewards, buf->dones,
                     (const long long *)buf->last, rewards, dones, (uint32_t)buf->n, buf->T);
  return launched(fn);
}

int oc_rollout_gae(const oc_rollout_buf *buf, const float *last_values, const float *last_dones, double gamma,
                   double gae_lambda, void *stream) {
  static const char fn[] = "oc_rollout_gae";
  if (const int rc = check_buf(fn, buf)) return rc;
  if (!buf->advantages || !buf->returns) return fail(fn, "NULL advantages / returns");
  if (!last_values || !last_dones) return fail(fn, "NULL input row");
  GaeArgs a{};
  a.rewards = buf->rewards, a.values = buf->values, a.episode_starts = buf->episode_starts;
  a.advantages = buf->advantages, a.returns = buf->returns;
  a.pos = (const long long *)buf->pos, a.count = (const long long *)buf->count;
  a.last_values = last_values, a.last_dones = last_dones;
  a.n = (uint32_t)buf->n, a.T = buf->T;
  a.g = (float)gamma;
  a.gl = (float)(gamma * gae_lambda);      // the product in double, as stable-baselines3 forms it
  const dim3 g((unsigned)((buf->n + 63) / 64)), b(64);
  hipLaunchKernelGGL(k_rollout_gae, g, b, 0, (hipStream_t)stream, a);
  return launched(fn);
}

}  // extern "C"
