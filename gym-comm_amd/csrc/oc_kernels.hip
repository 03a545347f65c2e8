// oc_kernels.hip -- the one translation unit of liboc_hip.so: hand-written CDNA4 (gfx950) kernels
// + the C ABI.  Three files:
//   oc_level_host.h   the host half of a level: LevelHdr / RunCfg and their one field list, the blob
//                     compiler (build_header), the text of a specialised header, the table image.
//                     Plain C++, compiled and run on its own by tests/test_host_cpu.py;
//   oc_step_device.h  the device code: everything from the per-env registers to the kernels;
//   this file         the launch policy (OC_LAUNCH), the table of kernel variants a library holds,
//                     the one launch helper and the extern "C" entry points.
//
// One lane = one environment; the env's whole dynamic state (A + M + 2 packed int32
// words, include/oc_hip.h) lives in VGPRs for the step.  All global tensors are
// env-major SoA, so every wave load/store touches 256 contiguous bytes.
//
// Everything that is the same for all envs of a launch (map bit-planes, subtask goal
// sets, item types, lookup programs for reward shaping) travels BY VALUE in the kernel
// argument block: it is read with scalar loads into SGPRs, costs no VGPRs, no LDS and
// no workgroup barrier, and makes every test on it a scalar branch.  The only tables a
// lane indexes with its own data -- the cell-to-cell path-distance table (u8) and the
// table of fp64 quotients k / MAX_PATH -- are read straight from global memory (2.4 KB +
// 2 KB, resident in every CU's vector L1 after first touch); the kernels were measured
// with those tables staged in LDS first (round-1 "v1", profiles/r01_v1_*) and the
// staging loop + barrier + LDS byte reads dominated the critical path at the BASELINE
// batch sizes, where only 1-2 waves per SIMD exist to hide latency.
//
// Control flow inside a step is branch-free on per-lane data: interact() is a decision
// phase (which of move / deliver / merge / chop / drop / pick fires) followed by
// predicated per-item updates; done/reward use a bitmask of "which goal object exists"
// instead of loops over subtasks.  Pure integer / indexing work; the fp64 shaping terms
// are table lookups plus adds in the reference's order (bit-exact).  No MFMA.
//
// Semantics follow the reference line by line (citations = paths relative to the
// reference root); the data model is our own: an Object is an equivalence class over M
// base items, each item carrying {cell, chopped, group, holder, world-order rank,
// type-set of its Object} in one register.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <type_traits>

#include "../../include/oc_hip.h"
#include "oc_level_host.h"   // LevelHdr, RunCfg, build_header, the spec-header text, the table image (plain C++)
#include "oc_step_device.h"  // the kernels

namespace {
constexpr bool sig_bits_agree() {
  for (int t = 0; t < OC_NTYPES; t++)
    if (item_sig_bit(false, t) != sig_of_type<false>(t) || item_sig_bit(true, t) != sig_of_type<true>(t)) return false;
  return true;
}
static_assert(sig_bits_agree(), "build_header and the kernels place an item's content type at the same bits");
}  // namespace

struct oc_level {
  LevelHdr hdr;
  RunCfg run;
  int32_t slot[OC_MAX_SUBTASKS];        // canonical bit of the caller's subtask s
  int32_t goal_index[OC_MAX_SUBTASKS];  // index of its distinct goal object (dup mode: where its count lives)
  void *dev_tables;    // the level's lane-indexed tables (oc_level_host.h: build_tables)
  int32_t n16;         // table bytes / 16 (rounded up)
  int32_t quot_bytes;
  int device;
};

// A map set (oc_mapset_create): K maps of this structure library's structure
struct oc_mapset {
  int32_t k;
  LevelHdr hdr;     // blob 0's: what the set shares -- S, M, the dup flag, the scatter count
  uint32_t play;    // RunCfg.play, equal across the set
  void *dev;        // K MapRecords, then the maps' table images (oc_step_device.h: MapRecord)
  int device;
};

// A prepared oc_multi_step (oc_multi_step_prepare): every argument by value
struct oc_call {
  const oc_level *lv;
  int32_t *state, *comm;
  const int32_t *actions;
  oc_wrap_cfg cfg;
  void *obs;
  double *timestep, *reward;
  int32_t *done, *sparse;
  int32_t auto_reset;
  int64_t *metrics;
  const int32_t *placement;
  uint32_t *rng;
  oc_step_opts opts;
  oc_step_policy pol[2];
  bool has_pol;
  int64_t n;
};

namespace {

thread_local char g_err[256] = "";

int fail(int code, const char *msg) {
  snprintf(g_err, sizeof(g_err), "%s", msg);
  return code;
}
int fail_hip(hipError_t e, const char *what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return (int)e;
}

// OC_TIMELINE builds: the launches that follow oc_timeline_begin() take consecutive records
#ifdef OC_TIMELINE
unsigned long long *g_timeline = nullptr;
int64_t g_timeline_left = 0, g_timeline_stride = 0;
#endif
// `waves`: an upper bound of the waves the launch will have
unsigned long long *timeline_next(int64_t waves, int64_t &stride) {
  stride = 0;
#ifdef OC_TIMELINE
  if (g_timeline_left > 0 && waves <= g_timeline_stride) {
    unsigned long long *r = g_timeline;
    g_timeline += 2 * g_timeline_stride;   // 16 bytes per wave
    g_timeline_left--;
    stride = g_timeline_stride;
    return r;
  }
#endif
  (void)waves;
  return nullptr;
}

// ---- launch policy ---------------------------------------------------------------------------
// ONE knob for measurements and tests forces what the library otherwise decides per call:
//   OC_LAUNCH="split=4,step_split=1,wt=0,lds=1,block=128"      (any subset, comma separated)
//     split       waves per 64 envs of the fused step (oc_multi_step): 1, 2 or 4     [split_for]
//     step_split  waves per 64 envs of the base step (oc_step): 1 or 2                [step_split_for]
//     wt          1 = write-through (sc1) stores, 0 = write-back                      [write_through]
//     lds         1 = the lane-indexed tables staged in LDS (one wave per 64 envs)    [tables_in_lds]
//     block       threads per workgroup of an unsplit launch: 64, 128 or 256          [block_size_for]
//     lanes       lanes per env of the fused step's plain four-way split: 1 or 2      [lanes_for]
// Read at EVERY call (a getenv and a string compare), so one process can run several policies --
// tests/test_hip_parity.py::test_forced_launch_policies does.  Results never depend on it.
// (Round 2 had six variables, three of them latched at first use; they are gone.)
struct LaunchPolicy {
  int split = 0, step_split = 0, wt = -1, lds = -1, block = 0, lanes = 0;
};
LaunchPolicy launch_policy() {
  static thread_local char seen[128] = "\x01";
  static thread_local LaunchPolicy cur;
  const char *v = getenv("OC_LAUNCH");
  if (!v) v = "";
  if (strncmp(v, seen, sizeof(seen)) == 0) return cur;
  snprintf(seen, sizeof(seen), "%s", v);
  LaunchPolicy p;
  for (const char *q = v; *q;) {
    int val = 0;
    char key[16] = "";
    int used = 0;
    if (sscanf(q, " %15[a-z_]=%d%n", key, &val, &used) == 2) {
      if (!strcmp(key, "split") && (val == 1 || val == 2 || val == 4)) p.split = val;
      else if (!strcmp(key, "step_split") && (val == 1 || val == 2)) p.step_split = val;
      else if (!strcmp(key, "wt") && (val == 0 || val == 1)) p.wt = val;
      else if (!strcmp(key, "lds") && (val == 0 || val == 1)) p.lds = val;
      else if (!strcmp(key, "block") && (val == 64 || val == 128 || val == 256)) p.block = val;
      else if (!strcmp(key, "lanes") && (val == 1 || val == 2)) p.lanes = val;
      q += used;
    }
    while (*q && *q != ',') q++;
    if (*q == ',') q++;
  }
  cur = p;
  return cur;
}

int block_size_for(int64_t) {
  // One wave per workgroup spreads a batch over the most CUs and measured fastest at every
  // batch size from 4 096 to 524 288 envs (MI355X sweeps, profiles/r01_v3_block_lds_sweep.txt,
  // r01_v11_geometry_sweep.txt).
  const int forced = launch_policy().block;
  return forced ? forced : 64;
}

// rows are addressed with 32-bit byte offsets through a buffer descriptor
bool fits_buffer(int64_t n, int64_t rows, int elem) { return n * rows * elem < (int64_t)0x7FFFFFFF; }

// The two shapes of a launch: unsplit -- one lane per env, block_size_for(n) threads per workgroup --
// and split -- sp waves per 64 envs, one workgroup each (k_step<..., SP = 2>, k_multi_step<..., SP =
// 2 / 4>).  `envs` is what the kernels' preloaded launch_ / block_ word carries in its low half.
struct Shape {
  int envs, threads;   // per workgroup
};
Shape shape_for(int64_t n, int sp, int ln = 1) {
  if (sp > 1) return {64 / ln, 64 * sp};   // (lane-split: ln lanes per env, 64 / ln envs per workgroup)
  const int bs = block_size_for(n);
  return {bs, bs};
}

// THE launch: ceil(n / envs) workgroups, range check, error check
template <typename K, typename... Args>
int launch(K kernel, Shape s, int64_t n, size_t lds_bytes, void *stream, const Args &...args) {
  if (n == 0) return OC_OK;
  const int64_t grid = (n + s.envs - 1) / s.envs;
  if (grid > 0x7FFFFFFF) return fail(OC_E_BADARG, "n too large");
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(s.threads), lds_bytes, (hipStream_t)stream, args...);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail_hip(e, "kernel launch");
  return OC_OK;
}

// Waves per 64 envs for the fused step (see multi_step_body): four up to 32 768 envs, one beyond.
// us per step, one / two / four waves per 64 envs (tools/ab_set.sh, MI355X, round-3 kernels --
// predicates as VALU words, ~4 cycles per instruction):
//   tomato-2  4 096 3.41 / - / 2.82   16 384 - / - / 2.95   32 768 - / 4.13 / 3.75   40 960 3.93 / - / 4.40
//             49 152 4.14 / - / 4.48   65 536 4.94 / 5.17 / 5.31   131 072 7.73 / - / -
//   salad-2   32 768 4.08 / 4.32 / 3.97
// (Round 2, at ~7 cycles per instruction: four up to 24 576, two up to 32 768 -- the two-way split
// no longer wins anywhere and is only launched on the caller's hint.)
// The caller's hint (oc_step_opts.waves_per_64 = 1 / 2 / 4) and OC_LAUNCH=split=... override.
int split_for(int64_t n, int hint) {
  const int forced = launch_policy().split;
  if (forced) return forced;
  if (hint == 1 || hint == 2 || hint == 4) return hint;
  return n <= 32768 ? 4 : 1;
}

// Lanes per env of the plain four-way split (k_multi_step<..., LN>, see LaneParts): two while the
// launch's 8 * n / 64 waves still find a SIMD of their own (1 024 on the chip), so that the extra
// waves run on CUs that would otherwise idle.  us per step, one / two / four lanes per env (MI355X,
// profiles/lane_split_ab.txt, medians of five alternating runs):
//   tomato-2  4 096 2.705 / 2.630 / 2.715   8 192 2.756 / 2.703 / 3.439   16 384 2.953 / 3.443 / 4.847
//             32 768 3.750 / 4.915 / 7.598   salad-2  32 768 3.958 / 4.967 / 7.715
// (four lanes per env never won and are not built).  OC_LAUNCH=lanes=... overrides; a library or
// variant without the kernel runs one lane per env (select_multi).
constexpr int64_t LANES2_MAX_N = 8192;
int lanes_for(int64_t n) {
  const int forced = launch_policy().lanes;
  if (forced) return forced;
  return n <= LANES2_MAX_N ? 2 : 1;
}

// The same for the base step (k_step<..., SP = 2>: state wave + shaping wave): two up to 16 384
// envs (tl-3: 16 384 3.44 -> 3.00 us, 24 576 3.51 / 3.97, 32 768 3.58 / 4.06, 65 536 3.82 / 4.38).
int step_split_for(int64_t n) {
  const int forced = launch_policy().step_split;
  if (forced) return forced;
  return n <= 16384 ? 2 : 1;
}

bool write_through(int64_t n) {
  // sc1 stores (see RowsT) at every batch size (tools/wt_threshold.sh)
  (void)n;
  const int forced = launch_policy().wt;
  return forced >= 0 ? forced == 1 : true;
}

bool tables_in_lds(int64_t) {
  // Off by default: with one- or two-wave workgroups the staging pass + barrier never paid
  // in the sweep (it only wins with 256-thread workgroups, which lose overall).
  // OC_LAUNCH=lds=1 selects the LDS variant (kept compiled, tested, and measured).
  return launch_policy().lds == 1;
}

// ---- which kernels this library holds ----------------------------------------------------------
// A kernel VARIANT is a plain struct of the template arguments a launch takes; for each kind of
// launch ONE function selects the variant (from the level, the caller's configuration and
// launch_policy()), ONE constexpr predicate `held` says whether this flavour of library holds it,
// and lift() turns the run-time values into template arguments.  The kernels a library contains are
// exactly the variants `held` admits, over the candidates listed here -- nothing else names them.
// What a specialised library (OC_SPECIALIZED: one (A, M, DUP), the level's) has and the generic one
// (every A in 2..4, M in 3..5, both DUP; its build time) has not: the fused step's two-way split,
// its four-way split of anything but the plain variant, XO = 1 (the options on the folded standard
// configuration), POL (both policies behind the step), and k_step on two waves.
template <typename T, T... Cs>
struct Among {   // a run-time value and the values it may take
  T v;
};
using Bool = Among<bool, false, true>;
using ObsType = Among<int, 0, 1, 2>;   // obs_int8: 0 int32, 1 int8, 2 float32
#ifdef OC_SPECIALIZED
constexpr bool SPEC = true;
using Agents = Among<int, OC_SPEC_HDR.A>;
using Items = Among<int, OC_SPEC_HDR.M>;
using Dup = Among<bool, OC_SPEC_HDR.has_dup != 0>;
constexpr const char *NO_AM = "specialised library built for another (num_agents, num_items)";
#else
constexpr bool SPEC = false;
using Agents = Among<int, 2, 3, 4>;
using Items = Among<int, 3, 4, 5>;
using Dup = Bool;
constexpr const char *NO_AM = "unsupported (num_agents, num_items): need A in 2..4, M in 3..5";
#endif
constexpr int NO_KERNEL = -1000;   // lift(): no candidate equals the value

// lift(f, Among{v}...) = f(std::integral_constant<T, v>{}...): a few compares per argument
template <auto... Vs, typename F>
int lift(F &&f) {
  return f(std::integral_constant<decltype(Vs), Vs>{}...);
}
template <auto... Vs, typename F, typename T, T... Cs, typename... Rest>
int lift(F &&f, Among<T, Cs...> a, Rest... rest) {
  int r = NO_KERNEL;
  (void)((a.v == Cs && (r = lift<Vs..., Cs>(f, rest...), true)) || ...);
  return r;
}
int no_kernel(int r, const char *msg) { return r == NO_KERNEL ? fail(OC_E_BADARG, msg) : r; }
// a variant the select function chose and `held` denies: the two have diverged (cannot happen)
int not_held() { return fail(OC_E_BADARG, "kernel variant not in this library (selection and held() disagree)"); }

// the base step, k_step<A, M, LDS, WT, DUP, PLAY, SP>
struct StepVariant {
  bool lds, wt, play;
  int sp;
};
constexpr bool held(StepVariant v) {
  if (v.lds) return !v.wt && v.sp == 1;
  return v.sp == 1 || (SPEC && v.wt && v.sp == 2);
}
StepVariant select_step(const oc_level *lv, int64_t n) {
  StepVariant v{tables_in_lds(n), false, lv->run.play != 0, 1};
  if (v.lds) return v;
  v.wt = write_through(n);
  if (v.wt) v.sp = step_split_for(n);
  if (!held(v)) v.sp = 1;
  return v;
}

// the fused step, k_multi_step<M, LDS, OT, WT, DUP, XO, SP, POL>.  XO: 0 = the plain variant (no
// options, the wrapper's standard configuration), 1 = options on the folded standard configuration,
// 2 = the general variant.
struct MultiVariant {
  int M;
  bool dup, lds;
  int ot;
  bool wt;
  int xo, sp;
  bool pol;
  int ln = 1;   // lanes per env
};
constexpr bool held(MultiVariant v) {
  if (v.xo == 1 && !SPEC) return false;
  if (v.ln != 1 && !(SPEC && v.ln == 2 && v.xo == 0 && v.sp == 4 && !v.pol && v.wt && !v.lds)) return false;
  if (v.lds) return v.ot == 0 && !v.wt && v.sp == 1 && !v.pol;   // (the split launches read global memory)
  if (v.pol) return SPEC && v.wt && v.xo == 1 && v.sp != 2;
  if (v.sp == 4) return v.wt && (SPEC || v.xo == 0);
  if (v.sp == 2) return SPEC && v.wt && v.xo == 0;
  return true;
}
// `general`: options in use or not the standard configuration `std_cfg`.  M and dup are the level's
// and select nothing else: the caller fills them in.
MultiVariant select_multi(int ot, bool general, bool std_cfg, bool pol, int hint, int64_t n) {
  MultiVariant v{0, false, false, ot, write_through(n), 0, 1, pol}, x1 = v;
  const bool in_lds = tables_in_lds(n);
  x1.xo = 1;
  if (general) v.xo = std_cfg && held(x1) ? 1 : 2;
  if (v.wt && !in_lds) v.sp = split_for(n, hint);   // the policy's wish ...
  if (!held(v)) v.sp = 1;                           // ... and what this library has kernels for
  v.ln = lanes_for(n);
  if (!held(v)) v.ln = 1;
  if (in_lds && ot == 0) v.lds = true, v.wt = false;   // (int8 / float32 rows: the global-table variant)
  return v;
}

}  // namespace

extern "C" {

int oc_abi_version(void) { return OC_ABI_VERSION; }
const char *oc_last_error(void) { return g_err; }

int oc_is_specialized(void) {
#if defined(OC_SPECIALIZED) && defined(OC_SPEC_GEOMETRY)
  return 2;   // a "level" library: structure and geometry folded
#elif defined(OC_SPECIALIZED)
  return 1;   // a "structure" library: geometry at run time
#else
  return 0;
#endif
}

int oc_level_spec_source(const int32_t *b, int32_t n_words, int32_t with_geometry, char *buf, int32_t buf_size) {
  LevelHdr full, h;
  RunCfg run;
  const char *msg = build_header(b, n_words, full, run);
  if (msg) {
    snprintf(g_err, sizeof(g_err), "oc_level_spec_source: %s", msg);
    return OC_E_BADARG;
  }
  // a "structure" library keeps the geometry a run-time argument: blank it in the header
  h = with_geometry ? full : structure_of(full);
  if (!buf || buf_size < 64) return fail(OC_E_BADARG, "oc_level_spec_source: buffer too small");
  const int n = spec_header_text(h, buf, buf_size);
  if (n >= buf_size) return fail(OC_E_BADARG, "oc_level_spec_source: buffer too small");
  return n;
}

int oc_level_create(const int32_t *b, int32_t n_words, oc_level_t **out) {
  if (!out) return fail(OC_E_BADARG, "oc_level_create: null out pointer");
  oc_level *lv = new (std::nothrow) oc_level();
  if (!lv) return fail(OC_E_BADARG, "oc_level_create: out of memory");
  lv->dev_tables = nullptr;
  LevelHdr &h = lv->hdr;
  const char *msg = build_header(b, n_words, h, lv->run, lv->slot, lv->goal_index);
  if (msg) {
    delete lv;
    snprintf(g_err, sizeof(g_err), "oc_level_create: %s", msg);
    return OC_E_BADARG;
  }
#ifdef OC_SPECIALIZED
  {
#ifdef OC_SPEC_GEOMETRY
    const LevelHdr spec = OC_SPEC_HDR, mine = h;
#else
    const LevelHdr spec = OC_SPEC_HDR, mine = structure_of(h);
#endif
    if (memcmp(&spec, &mine, sizeof(LevelHdr)) != 0) {
      delete lv;
      return fail(OC_E_BADARG, "oc_level_create: this library is specialised for a different level (a \"level\" "
                               "library) or level structure (recipes, item multiset, agent count, border kind)");
    }
  }
#endif
  std::vector<uint8_t> img;
  try {
    msg = build_tables(b, h, img);
  } catch (const std::bad_alloc &) {
    msg = "out of memory";
  }
  if (msg) {
    delete lv;
    snprintf(g_err, sizeof(g_err), "oc_level_create: %s", msg);
    return OC_E_BADARG;
  }
  const size_t bytes = img.size();
  lv->quot_bytes = 0;
  lv->n16 = (int32_t)(bytes / 16);
  hipError_t e = hipGetDevice(&lv->device);
  if (e == hipSuccess) e = hipMalloc(&lv->dev_tables, bytes);
  if (e == hipSuccess) e = hipMemcpy(lv->dev_tables, img.data(), bytes, hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    oc_level_destroy(lv);
    fail_hip(e, "oc_level_create");
    return OC_E_NODEVICE;
  }
  *out = lv;
  return OC_OK;
}

int oc_level_destroy(oc_level_t *lv) {
  if (!lv) return OC_OK;
  if (lv->dev_tables) (void)hipFree(lv->dev_tables);
  delete lv;
  return OC_OK;
}

int oc_level_subtask_info(const int32_t *b, int32_t n_words, int32_t *slot, int32_t *goal_index, int32_t *dup) {
  LevelHdr h;
  RunCfg run;
  int32_t sl[OC_MAX_SUBTASKS], gi[OC_MAX_SUBTASKS];
  const char *msg = build_header(b, n_words, h, run, sl, gi);
  if (msg) {
    snprintf(g_err, sizeof(g_err), "oc_level_subtask_info: %s", msg);
    return OC_E_BADARG;
  }
  for (int s = 0; s < h.S; s++) {
    if (slot) slot[s] = sl[s];
    if (goal_index) goal_index[s] = gi[s];
  }
  if (dup) *dup = (int32_t)h.has_dup;
  return OC_OK;
}

// One slot per wave of 64 envs, rounded up to whole workgroups of four waves: under a forced
// 128- / 256-thread workgroup (OC_LAUNCH=block=...) the last workgroup may hold waves without an env,
// and those add zeros to THEIR slot.
int64_t oc_metrics_slots(int64_t n) { return n <= 0 ? 0 : (n + 255) / 256 * 4; }
int32_t oc_state_words(const oc_level_t *lv) {
  return lv ? lv->hdr.A + lv->hdr.M + 2 + (lv->hdr.has_dup ? 2 : 0) : 0;
}
int32_t oc_obs_rows(const oc_level_t *lv, int32_t num_comm) {
  return lv ? 22 + lv->hdr.S + 2 * num_comm : 0;
}

int oc_reset(const oc_level_t *lv, int32_t *state, const int32_t *mask, const int32_t *placement, uint32_t *rng,
             int64_t n, void *stream) {
  if (lv && n == 0) return OC_OK;
  if (!lv || !state || n < 0) return fail(OC_E_BADARG, "oc_reset: bad argument");
  if (lv->hdr.nscatter > 0 && !placement && !rng)
    return fail(OC_E_BADARG, "oc_reset: this level places items at random; pass `placement` or `rng`");
  ResetArgs a{lv->hdr, lv->dev_tables, lv->n16, lv->quot_bytes, state, mask, placement, rng, n};
  return no_kernel(lift([&](auto A, auto M, auto D) { return launch(k_reset<A, M, D>, shape_for(n, 1), n, 0, stream, a); },
                        Agents{lv->hdr.A}, Items{lv->hdr.M}, Dup{lv->hdr.has_dup != 0}),
                   NO_AM);
}

int oc_step(const oc_level_t *lv, int32_t *state, const int32_t *actions, int32_t *reward, int32_t *done,
            double *shaping, int32_t auto_reset, int64_t *metrics, const int32_t *placement, uint32_t *rng,
            int64_t n, void *stream) {
  if (lv && n == 0) return OC_OK;
  if (!lv || !state || !actions || !reward || !done || !shaping || n < 0)
    return fail(OC_E_BADARG, "oc_step: bad argument");
  if (!fits_buffer(n, oc_state_words(lv), 4) || !fits_buffer(n, 2, 8))
    return fail(OC_E_BADARG, "oc_step: n too large for one call (tensor rows are addressed with 32-bit offsets); split the batch");
  if (auto_reset && lv->hdr.nscatter > 0 && !placement && !rng)
    return fail(OC_E_BADARG, "oc_step: auto_reset on a random-placement level needs `placement` or `rng`");
  StepArgs a{lv->hdr, lv->run, lv->dev_tables, lv->n16, lv->quot_bytes, state, actions, reward, done, shaping,
             metrics, placement, rng, n, auto_reset, nullptr, 0};
  a.timeline = timeline_next(4 * ((n + 63) / 64), a.timeline_stride);
  const StepVariant v = select_step(lv, n);
  const Shape shape = shape_for(n, v.sp);
  const int32_t launch_ = shape.envs | ((auto_reset ? 1 : 0) << 16);
  // hot scalars first (preloaded kernel arguments), then the full block
  return no_kernel(lift([&](auto A, auto M, auto D, auto LDS, auto WT, auto PLAY, auto SP) {
                          if constexpr (held(StepVariant{LDS, WT, PLAY, SP}))
                            return launch(k_step<A, M, LDS, WT, D, PLAY, SP>, shape, n, v.lds ? (size_t)lv->n16 * 16 : 0,
                                          stream, a.state, a.actions, a.metrics, a.n, launch_, a.R.T, a.tables,
                                          a.R.inv_max_path, a);
                          else
                            return not_held();
                        },
                        Agents{lv->hdr.A}, Items{lv->hdr.M}, Dup{lv->hdr.has_dup != 0}, Bool{v.lds}, Bool{v.wt},
                        Bool{v.play}, Among<int, 1, 2>{v.sp}),
                   NO_AM);
}

int oc_obs(const oc_level_t *lv, const int32_t *state, const int32_t *comm, const oc_obs_cfg *cfg,
           void *obs, double *timestep, int64_t n, void *stream) {
  if (lv && cfg && n == 0) return OC_OK;
  if (!lv || !state || !comm || !cfg || !obs || !timestep || n < 0 || cfg->num_comm < 0 || cfg->num_comm > 128)
    return fail(OC_E_BADARG, "oc_obs: bad argument");
  if (!fits_buffer(n, 2 * (22 + lv->hdr.S + 2 * cfg->num_comm), 4))
    return fail(OC_E_BADARG, "oc_obs: n too large for one call (tensor rows are addressed with 32-bit offsets); split the batch");
  ObsArgs a{lv->hdr, lv->run, state, comm, obs, timestep, n, *cfg};
  if (cfg->obs_int8 < 0 || cfg->obs_int8 > 2) return fail(OC_E_BADARG, "oc_obs: obs_int8 must be 0 (int32), 1 (int8) or 2 (float32)");
  // k_obs<A, M, OT, WT, DUP>: every library holds every (OT, WT)
  return no_kernel(lift([&](auto A, auto M, auto D, auto OT, auto WT) {
                          return launch(k_obs<A, M, OT, WT, D>, shape_for(n, 1), n, 0, stream, a);
                        },
                        Agents{lv->hdr.A}, Items{lv->hdr.M}, Dup{lv->hdr.has_dup != 0}, ObsType{cfg->obs_int8},
                        Bool{write_through(n)}),
                   NO_AM);
}

int32_t oc_image_words(const oc_level_t *lv) { return lv ? 7 * ((lv->hdr.ncells + 3) / 4) : 0; }

int oc_obs_image(const oc_level_t *lv, const int32_t *state, int32_t radius, int32_t *out, int8_t *holding,
                 int64_t n, void *stream) {
  if (lv && n == 0) return OC_OK;
  if (!lv || !state || !out || !holding || n < 0) return fail(OC_E_BADARG, "oc_obs_image: bad argument");
  if (!fits_buffer(n, 2 * oc_image_words(lv), 4))
    return fail(OC_E_BADARG, "oc_obs_image: n too large for one call; split the batch");
  ImageArgs a{lv->hdr, state, out, holding, n, radius};
  return no_kernel(lift([&](auto A, auto M, auto D) { return launch(k_obs_image<A, M, D>, shape_for(n, 1), n, 0, stream, a); },
                        Agents{lv->hdr.A}, Items{lv->hdr.M}, Dup{lv->hdr.has_dup != 0}),
                   NO_AM);
}

int oc_multi_step(const oc_level_t *lv, int32_t *state, int32_t *comm, const int32_t *actions,
                  const oc_wrap_cfg *cfg, void *obs, double *timestep, double *reward, int32_t *done,
                  int32_t *sparse, int32_t auto_reset, int64_t *metrics, const int32_t *placement, uint32_t *rng,
                  const oc_step_opts *opts, int64_t n, void *stream) {
  if (lv && cfg && n == 0) return OC_OK;
  oc_step_opts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if ((o.ep_return == nullptr) != (o.ep_length == nullptr))
    return fail(OC_E_BADARG, "oc_multi_step: pass both ep_return and ep_length, or neither");
  // the action rows may only be absent when both players' actions come from somewhere else
  if (!actions && !(o.ego_pairs && (o.alt_pairs || o.alt_rng)))
    return fail(OC_E_BADARG, "oc_multi_step: no `actions` and no complete replacement in `opts`");
  if (!lv || !state || !comm || !cfg || !obs || !timestep || !reward || !done || n < 0 ||
      cfg->obs.num_comm < 0 || cfg->obs.num_comm > 128)
    return fail(OC_E_BADARG, "oc_multi_step: bad argument");
  if (lv->hdr.A != 2)
    return fail(OC_E_BADARG, "oc_multi_step: the gym_comm wrapper drives exactly 2 agents");
  if (!fits_buffer(n, 2 * (22 + lv->hdr.S + 2 * cfg->obs.num_comm), 4) || !fits_buffer(n, 1, 16))
    return fail(OC_E_BADARG, "oc_multi_step: n too large for one call (tensor rows are addressed with 32-bit offsets); split the batch");
  if (auto_reset && lv->hdr.nscatter > 0 && !placement && !rng)
    return fail(OC_E_BADARG, "oc_multi_step: auto_reset on a random-placement level needs `placement` or `rng`");
  MultiArgs a{lv->hdr, lv->run, lv->dev_tables, lv->n16, lv->quot_bytes, state, comm, actions, obs, timestep,
              reward, done, sparse, metrics, placement, rng, o, n, auto_reset, *cfg, {}, 0, nullptr, 0};
  if (o.policy) {   // the closed loop in one launch (oc_step_opts.policy)
#ifndef OC_SPECIALIZED
    return fail(OC_E_BADARG, "oc_multi_step: opts.policy needs a specialised library (this is the generic one)");
#endif
    if (!o.ego_pairs || !o.alt_pairs || o.pairs_int64 || o.alt_rng)
      return fail(OC_E_BADARG, "oc_multi_step: opts.policy needs ego_pairs and alt_pairs (int32) and no alt_rng");
    if (cfg->obs.num_comm < 1 || cfg->obs.num_comm > 4)
      return fail(OC_E_BADARG, "oc_multi_step: opts.policy samples at most 4 comm channels; use oc_policy_mlp");
    for (int k = 0; k < 2; k++) {
      if (!o.policy[k].w1 || !o.policy[k].w2 || !o.policy[k].b2)
        return fail(OC_E_BADARG, "oc_multi_step: opts.policy[k] needs w1, w2 and b2");
      a.pol[k] = o.policy[k];
    }
    a.pol_ksteps = (22 + lv->hdr.S + 2 * cfg->obs.num_comm + 2 + 15) / 16;
    if (a.pol_ksteps > 3)
      return fail(OC_E_BADARG, "oc_multi_step: opts.policy handles at most 46 observation rows; use oc_policy_mlp");
    a.opt.policy = nullptr;   // (a host pointer: nothing on the device may look at it)
  }
  a.timeline = timeline_next(4 * ((n + 63) / 64), a.timeline_stride);
  const int ot = cfg->obs.obs_int8;   // 0 int32, 1 int8, 2 float32
  if (ot < 0 || ot > 2) return fail(OC_E_BADARG, "oc_multi_step: obs_int8 must be 0 (int32), 1 (int8) or 2 (float32)");
  const bool std_cfg = cfg->communication_on && !cfg->ego_led && cfg->can_move_mask == 3 &&
                       cfg->ego_agent_idx == 0 && cfg->obs.blind_mask == 0 && !lv->run.play;
  const bool opts_used = o.ep_return || o.ego_pairs || o.alt_pairs || o.alt_rng;
  if (o.policy && !std_cfg)
    return fail(OC_E_BADARG, "oc_multi_step: opts.policy runs on the wrapper's standard configuration (communication on, "
                             "not ego-led, both CAN_MOVE, ego_agent_idx 0, nobody BLIND, play off); use oc_policy_mlp + oc_multi_step");
  if (o.policy && (!write_through(n) || tables_in_lds(n)))
    return fail(OC_E_BADARG, "oc_multi_step: opts.policy needs write-through stores and tables in global memory");
  MultiVariant v = select_multi(ot, opts_used || !std_cfg, std_cfg, o.policy != nullptr, o.waves_per_64, n);
  v.M = lv->hdr.M, v.dup = lv->hdr.has_dup != 0;
  const Shape shape = shape_for(n, v.sp, v.ln);
  // the hot scalars lead (see k_multi_step): block_ = envs per workgroup | action sources in use << 16
  const int32_t src = (o.ego_pairs ? 1 : 0) | (o.alt_pairs ? 2 : 0) | (o.alt_rng ? 4 : 0) | (o.pairs_int64 ? 8 : 0);
  const int32_t block_ = shape.envs | (src << 16);
  const void *const alt_src = o.alt_rng ? (const void *)o.alt_rng : (const void *)o.alt_pairs;
  return no_kernel(lift([&](auto M, auto D, auto LDS, auto OT, auto WT, auto XO, auto SP, auto POL, auto LN) {
                          if constexpr (held(MultiVariant{M, D, LDS, OT, WT, XO, SP, POL, LN}))
                            return launch(k_multi_step<M, LDS, OT, WT, D, XO, SP, POL, LN>, shape, n,
                                          v.lds ? (size_t)lv->n16 * 16 : 0, stream, a.state, a.actions, a.comm, a.metrics,
                                          (int32_t)a.n, block_, (const void *)o.ego_pairs, alt_src, a);
                          else
                            return not_held();
                        },
                        Items{v.M}, Dup{v.dup}, Bool{v.lds}, ObsType{v.ot}, Bool{v.wt}, Among<int, 0, 1, 2>{v.xo},
                        Among<int, 1, 2, 4>{v.sp}, Bool{v.pol}, Among<int, 1, 2>{v.ln}),
                   "oc_multi_step: unsupported number of items");
}

int oc_multi_step_prepare(const oc_level_t *lv, int32_t *state, int32_t *comm, const int32_t *actions,
                          const oc_wrap_cfg *cfg, void *obs, double *timestep, double *reward, int32_t *done,
                          int32_t *sparse, int32_t auto_reset, int64_t *metrics, const int32_t *placement,
                          uint32_t *rng, const oc_step_opts *opts, int64_t n, oc_call_t **out) {
  if (!out || !lv || !cfg) return fail(OC_E_BADARG, "oc_multi_step_prepare: bad argument");
  oc_call *c = new (std::nothrow) oc_call();
  if (!c) return fail(OC_E_BADARG, "oc_multi_step_prepare: out of memory");
  c->lv = lv, c->state = state, c->comm = comm, c->actions = actions, c->cfg = *cfg, c->obs = obs;
  c->timestep = timestep, c->reward = reward, c->done = done, c->sparse = sparse, c->auto_reset = auto_reset;
  c->metrics = metrics, c->placement = placement, c->rng = rng, c->n = n;
  memset(&c->opts, 0, sizeof(c->opts));
  if (opts) c->opts = *opts;
  c->has_pol = c->opts.policy != nullptr;
  if (c->has_pol) {   // (a host array of the caller: copied, so that it need not outlive this call)
    c->pol[0] = c->opts.policy[0], c->pol[1] = c->opts.policy[1];
    c->opts.policy = c->pol;
  }
  *out = c;
  return OC_OK;
}

int oc_call_launch(const oc_call_t *c, const void *ego_pairs, int32_t pairs_int64, void *stream) {
  if (!c) return fail(OC_E_BADARG, "oc_call_launch: null call");
  oc_step_opts o = c->opts;
  if (ego_pairs) {
    o.ego_pairs = (const int32_t *)ego_pairs;
    o.pairs_int64 = pairs_int64;
  }
  return oc_multi_step(c->lv, c->state, c->comm, c->actions, &c->cfg, c->obs, c->timestep, c->reward, c->done,
                       c->sparse, c->auto_reset, c->metrics, c->placement, c->rng, &o, c->n, stream);
}

int oc_call_destroy(oc_call_t *c) {
  delete c;
  return OC_OK;
}

int oc_timeline_begin(uint64_t *records, int64_t count, int64_t stride) {
#ifdef OC_TIMELINE
  if ((records == nullptr) != (count == 0) || count < 0 || (count > 0 && stride < 1))
    return fail(OC_E_BADARG, "oc_timeline_begin: bad argument");
  g_timeline = (unsigned long long *)records;
  g_timeline_left = count;
  g_timeline_stride = stride;
  return OC_OK;
#else
  (void)records;
  (void)count;
  (void)stride;
  return fail(OC_E_BADARG, "oc_timeline_begin: not a timeline build of the library (-DOC_TIMELINE)");
#endif
}

int32_t oc_multi_step_waves(int64_t n, int32_t hint, int32_t general_variant) {
  return select_multi(0, general_variant != 0, false, false, hint, n).sp;
}

int32_t oc_multi_step_lanes(int64_t n, int32_t hint, int32_t general_variant) {
  return select_multi(0, general_variant != 0, false, false, hint, n).ln;
}

// ---- map sets (structure libraries; oc_step_device.h: k_mapset_*) -------------------------------
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
namespace {
int fail_at(int index, const char *what, const char *msg) {
  snprintf(g_err, sizeof(g_err), "%s: blob %d: %s", what, index, msg);
  return OC_E_BADARG;
}
// a set launch: always one group of 64 envs per workgroup, on `sp` waves
Shape set_shape(int sp) { return {64, 64 * sp}; }
// Waves per 64 envs of a set's fused step: the policy's or the caller's wish (split_for), brought to
// the nearest launch the set kernels have -- one wave, or the four-way split (two -> four)
int set_split_for(int64_t n, int hint) { return split_for(n, hint) == 1 ? 1 : 4; }
}  // namespace
#endif

int oc_mapset_create(const int32_t *const *blobs, const int32_t *n_words, int32_t k, oc_mapset_t **out) {
#if !defined(OC_SPECIALIZED)
  (void)blobs, (void)n_words, (void)k, (void)out;
  return fail(OC_E_BADARG, "oc_mapset_create: map sets need a structure library (this is the generic one)");
#elif defined(OC_SPEC_GEOMETRY)
  (void)blobs, (void)n_words, (void)k, (void)out;
  return fail(OC_E_BADARG, "oc_mapset_create: map sets need a structure library (this is a level library: one map folded in)");
#else
  if (!out || !blobs || !n_words) return fail(OC_E_BADARG, "oc_mapset_create: null pointer");
  if (k < 1) return fail(OC_E_BADARG, "oc_mapset_create: a map set holds at least one map (k < 1)");
  std::vector<MapRecord> recs;
  std::vector<uint8_t> image, img;
  oc_mapset *ms = nullptr;
  try {
    recs.resize((size_t)k);
    const size_t rec_bytes = ((size_t)k * sizeof(MapRecord) + 15) & ~(size_t)15;
    image.assign(rec_bytes, 0);
    for (int32_t m = 0; m < k; m++) {
      MapRecord &r = recs[(size_t)m];
      memset(&r, 0, sizeof(r));
      const char *msg = build_header(blobs[m], n_words[m], r.L, r.R);
      if (msg) return fail_at(m, "oc_mapset_create", msg);
      const LevelHdr spec = OC_SPEC_HDR, mine = structure_of(r.L), first = structure_of(recs[0].L);
      if (memcmp(&spec, &mine, sizeof(LevelHdr)) != 0)
        return fail_at(m, "oc_mapset_create", "its structure (recipes, item multiset, agent count, border kind) is not this library's");
      if (memcmp(&first, &mine, sizeof(LevelHdr)) != 0)
        return fail_at(m, "oc_mapset_create", "its structure differs from blob 0's");
      if (r.L.A != 2) return fail_at(m, "oc_mapset_create", "map sets step exactly 2 agents");
      if (r.R.slot_identity != recs[0].R.slot_identity || memcmp(r.R.slot4, recs[0].R.slot4, sizeof(r.R.slot4)) != 0)
        return fail_at(m, "oc_mapset_create", "its subtask order differs from blob 0's");
      if (r.R.play != recs[0].R.play) return fail_at(m, "oc_mapset_create", "its `play` flag differs from blob 0's");
      msg = build_tables(blobs[m], r.L, img);
      if (msg) return fail_at(m, "oc_mapset_create", msg);
      r.tab_off = (int64_t)image.size();
      r.n16 = (int32_t)(img.size() / 16);
      image.insert(image.end(), img.begin(), img.end());   // (a multiple of 16 bytes: every image stays aligned)
    }
    ms = new oc_mapset();
  } catch (const std::bad_alloc &) {
    return fail(OC_E_BADARG, "oc_mapset_create: out of memory");
  }
  ms->k = k;
  ms->hdr = recs[0].L;
  ms->play = recs[0].R.play;
  ms->dev = nullptr;
  hipError_t e = hipGetDevice(&ms->device);
  if (e == hipSuccess) e = hipMalloc(&ms->dev, image.size());
  if (e == hipSuccess) {   // (the records carry their table image's device address)
    for (int32_t m = 0; m < k; m++) recs[(size_t)m].tables = (const char *)ms->dev + recs[(size_t)m].tab_off;
    memcpy(image.data(), recs.data(), (size_t)k * sizeof(MapRecord));
    e = hipMemcpy(ms->dev, image.data(), image.size(), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    oc_mapset_destroy(ms);
    fail_hip(e, "oc_mapset_create");
    return OC_E_NODEVICE;
  }
  *out = ms;
  return OC_OK;
#endif
}

int oc_mapset_destroy(oc_mapset_t *ms) {
  if (!ms) return OC_OK;
  if (ms->dev) (void)hipFree(ms->dev);
  delete ms;
  return OC_OK;
}

int oc_mapset_reset(const oc_mapset_t *ms, const int32_t *group_map, int32_t *state, const int32_t *mask,
                    const int32_t *placement, uint32_t *rng, int64_t n, void *stream) {
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
  if (ms && group_map && n == 0) return OC_OK;
  if (!ms || !group_map || !state || n < 0) return fail(OC_E_BADARG, "oc_mapset_reset: bad argument");
  if (ms->hdr.nscatter > 0 && !placement && !rng)
    return fail(OC_E_BADARG, "oc_mapset_reset: these maps place items at random; pass `placement` or `rng`");
  const SetResetArgs a{(const MapRecord *)ms->dev, group_map, state, mask, placement, rng, n};
  return no_kernel(lift([&](auto M, auto D) { return launch(k_mapset_reset<M, D>, set_shape(1), n, 0, stream, a); },
                        Items{ms->hdr.M}, Dup{ms->hdr.has_dup != 0}),
                   NO_AM);
#else
  (void)ms, (void)group_map, (void)state, (void)mask, (void)placement, (void)rng, (void)n, (void)stream;
  return fail(OC_E_BADARG, "oc_mapset_reset: map sets need a structure library");
#endif
}

int oc_mapset_obs(const oc_mapset_t *ms, const int32_t *group_map, const int32_t *state, const int32_t *comm,
                  const oc_obs_cfg *cfg, void *obs, double *timestep, int64_t n, void *stream) {
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
  if (ms && group_map && cfg && n == 0) return OC_OK;
  if (!ms || !group_map || !state || !comm || !cfg || !obs || !timestep || n < 0 || cfg->num_comm < 0 ||
      cfg->num_comm > 128)
    return fail(OC_E_BADARG, "oc_mapset_obs: bad argument");
  if (!fits_buffer(n, 2 * (22 + ms->hdr.S + 2 * cfg->num_comm), 4))
    return fail(OC_E_BADARG, "oc_mapset_obs: n too large for one call (tensor rows are addressed with 32-bit offsets); split the batch");
  if (cfg->obs_int8 < 0 || cfg->obs_int8 > 2)
    return fail(OC_E_BADARG, "oc_mapset_obs: obs_int8 must be 0 (int32), 1 (int8) or 2 (float32)");
  const SetObsArgs a{(const MapRecord *)ms->dev, group_map, state, comm, obs, timestep, n, *cfg};
  return no_kernel(lift([&](auto M, auto D, auto OT) { return launch(k_mapset_obs<M, OT, D>, set_shape(1), n, 0, stream, a); },
                        Items{ms->hdr.M}, Dup{ms->hdr.has_dup != 0}, ObsType{cfg->obs_int8}),
                   NO_AM);
#else
  (void)ms, (void)group_map, (void)state, (void)comm, (void)cfg, (void)obs, (void)timestep, (void)n, (void)stream;
  return fail(OC_E_BADARG, "oc_mapset_obs: map sets need a structure library");
#endif
}

int oc_mapset_multi_step(const oc_mapset_t *ms, const int32_t *group_map, int32_t *state, int32_t *comm,
                         const int32_t *actions, const oc_wrap_cfg *cfg, void *obs, double *timestep,
                         double *reward, int32_t *done, int32_t *sparse, int32_t auto_reset, int64_t *metrics,
                         const int32_t *placement, uint32_t *rng, const oc_step_opts *opts, int64_t n,
                         void *stream) {
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
  if (ms && group_map && cfg && n == 0) return OC_OK;
  oc_step_opts o;
  memset(&o, 0, sizeof(o));
  if (opts) o = *opts;
  if ((o.ep_return == nullptr) != (o.ep_length == nullptr))
    return fail(OC_E_BADARG, "oc_mapset_multi_step: pass both ep_return and ep_length, or neither");
  if (!actions && !(o.ego_pairs && (o.alt_pairs || o.alt_rng)))
    return fail(OC_E_BADARG, "oc_mapset_multi_step: no `actions` and no complete replacement in `opts`");
  if (!ms || !group_map || !state || !comm || !cfg || !obs || !timestep || !reward || !done || n < 0 ||
      cfg->obs.num_comm < 0 || cfg->obs.num_comm > 128)
    return fail(OC_E_BADARG, "oc_mapset_multi_step: bad argument");
  if (o.policy) return fail(OC_E_BADARG, "oc_mapset_multi_step: opts.policy (the fused policies) is not available for map sets");
  if (!fits_buffer(n, 2 * (22 + ms->hdr.S + 2 * cfg->obs.num_comm), 4) || !fits_buffer(n, 1, 16))
    return fail(OC_E_BADARG, "oc_mapset_multi_step: n too large for one call (tensor rows are addressed with 32-bit offsets); split the batch");
  if (auto_reset && ms->hdr.nscatter > 0 && !placement && !rng)
    return fail(OC_E_BADARG, "oc_mapset_multi_step: auto_reset on random-placement maps needs `placement` or `rng`");
  const int ot = cfg->obs.obs_int8;
  if (ot < 0 || ot > 2) return fail(OC_E_BADARG, "oc_mapset_multi_step: obs_int8 must be 0 (int32), 1 (int8) or 2 (float32)");
  const MapRecord *maps = (const MapRecord *)ms->dev;
  const bool std_cfg = cfg->communication_on && !cfg->ego_led && cfg->can_move_mask == 3 &&
                       cfg->ego_agent_idx == 0 && cfg->obs.blind_mask == 0 && !ms->play;
  if (!std_cfg)
    return fail(OC_E_BADARG, "oc_mapset_multi_step: map sets run the wrapper's standard configuration (communication on, "
                             "not ego-led, both CAN_MOVE, ego_agent_idx 0, nobody BLIND, play off)");
  const int xo = (o.ep_return || o.ego_pairs || o.alt_pairs || o.alt_rng) ? 1 : 0;
  const int sp = set_split_for(n, o.waves_per_64);
  const SetMultiArgs a{maps, group_map, obs, timestep, reward, done, sparse, placement, rng, o, n, auto_reset, *cfg};
  const int32_t src = (o.ego_pairs ? 1 : 0) | (o.alt_pairs ? 2 : 0) | (o.alt_rng ? 4 : 0) | (o.pairs_int64 ? 8 : 0);
  const int32_t block_ = 64 | (src << 16);
  const void *const alt_src = o.alt_rng ? (const void *)o.alt_rng : (const void *)o.alt_pairs;
  return no_kernel(lift([&](auto M, auto D, auto OT, auto XO, auto SP) {
                          return launch(k_mapset_step<M, OT, D, XO, SP>, set_shape(sp), n, 0, stream, state, actions, comm,
                                        metrics, (int32_t)n, block_, (const void *)o.ego_pairs, alt_src, a);
                        },
                        Items{ms->hdr.M}, Dup{ms->hdr.has_dup != 0}, ObsType{ot}, Among<int, 0, 1>{xo},
                        Among<int, 1, 4>{sp}),
                   "oc_mapset_multi_step: unsupported number of items");
#else
  (void)ms, (void)group_map, (void)state, (void)comm, (void)actions, (void)cfg, (void)obs, (void)timestep, (void)reward;
  (void)done, (void)sparse, (void)auto_reset, (void)metrics, (void)placement, (void)rng, (void)opts, (void)n, (void)stream;
  return fail(OC_E_BADARG, "oc_mapset_multi_step: map sets need a structure library");
#endif
}

int32_t oc_mapset_multi_step_waves(int64_t n, int32_t hint, int32_t general_variant) {
  (void)general_variant;   // (XO = 0 and 1 have the same launches)
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
  return set_split_for(n, hint);
#else
  (void)n, (void)hint;
  return 0;   // no set kernels in this library
#endif
}

int oc_random_actions(uint32_t *rng, int32_t *move_row, int32_t *comm_row, int32_t num_comm, int64_t n,
                      void *stream) {
  if (n == 0 && rng && move_row && comm_row) return OC_OK;
  if (!rng || !move_row || !comm_row || n < 0 || num_comm < 1)
    return fail(OC_E_BADARG, "oc_random_actions: bad argument");
  return launch(k_random_actions, Shape{256, 256}, n, 0, stream, rng, move_row, comm_row, (uint32_t)num_comm, n);
}

}  // extern "C"
