// oc_policy.hip -- liboc_policy.so: a 64-unit tanh MLP policy on the observation rows of the
// batched Overcooked stepper, sampled into (move, comm) pairs (include/oc_policy.h).
//
// gfx950 only.  One wave = one PASS of 32 envs (oc_policy_device.h: both products on the matrix
// cores); two waves per workgroup, XCD-aware grid (k_policy_mlp below).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/oc_policy.h"
#include "oc_policy_device.h"
#include "oc_policy_ac_device.h"
#include "oc_policy_fail.h"
#include "oc_policy_layout.h"

// the library's last-error text (oc_policy_fail.h)
static thread_local char g_err[256] = "";
int ocpol::fail(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}

namespace {

struct Args {
  oc_policy_player pl[2];
  const double *timestep;
  int32_t F, C, ksteps;
  int64_t n;
};

using namespace ocpol;

// Workgroup -> envs, XCD-aware.  WPB = 2 (the shipped mapping): a workgroup is 64 envs, workgroup x
// of a player = envs 64 x .. 64 x + 63 -- the step kernels' mapping -- and the grid is one-
// dimensional with every player's range padded to a multiple of 8 workgroups (`gx8`), so that
// workgroup x of EVERY player runs on XCD x % 8 (workgroups are dealt to the 8 XCDs round-robin):
// the observation rows a workgroup reads were written, a launch earlier, through the L2 of its
// own XCD.  With 32-env workgroups in launch order (WPB = 1, kept for the A/B) a closed-loop step
// cost more than its two kernels apart: 28.5 us against 21.3 at 131 072 envs; matched: 22.2.
template <int OT, int WPB, int CMAX>
__global__ void __launch_bounds__(64 * WPB) k_policy_mlp(const Args p, const int gx, const int gx8) {
  const int x = (int)(blockIdx.x % (unsigned)gx8), y = (int)(blockIdx.x / (unsigned)gx8);
  if (x >= gx) return;                       // padding workgroup (uniform)
  const oc_policy_player &P = p.pl[y];
  const int lane = threadIdx.x & 63, r = lane & 31;
  const int64_t env0 = ((int64_t)x * WPB + (threadIdx.x >> 6)) * 32 + r;
  const bool valid = env0 < p.n;
  const int64_t env = valid ? env0 : p.n - 1;   // lanes past the batch compute on the last env, store nothing
  policy_pass<OT, CMAX>(P.obs, (uint32_t)p.n, (uint32_t)env, valid, lane, P.w1, P.w2, P.b2, P.rng, P.pairs, P.logits,
                        (float)p.timestep[env], p.F, p.C, p.ksteps);
}

// The actor-critic launch (oc_policy_mlp_ac): k_policy_mlp's grid and mapping, the tail of
// oc_policy_ac_device.h behind the same two products.
struct AcArgs {
  oc_policy_ac_player pl[2];
  const double *timestep;
  int32_t F, C, ksteps;
  int64_t n;
};

template <int OT, int WPB, int CMAX>
__global__ void __launch_bounds__(64 * WPB) k_policy_mlp_ac(const AcArgs p, const int gx, const int gx8) {
  const int x = (int)(blockIdx.x % (unsigned)gx8), y = (int)(blockIdx.x / (unsigned)gx8);
  if (x >= gx) return;                       // padding workgroup (uniform)
  const oc_policy_ac_player &A = p.pl[y];
  const oc_policy_player &P = A.p;
  const int lane = threadIdx.x & 63, r = lane & 31;
  const int64_t env0 = ((int64_t)x * WPB + (threadIdx.x >> 6)) * 32 + r;
  const bool valid = env0 < p.n;
  const int64_t env = valid ? env0 : p.n - 1;   // lanes past the batch compute on the last env, store nothing
  const AcTail tail = {A.given, A.move_row, A.comm_row, A.log_prob, A.value};
  policy_pass<OT, CMAX, false, false, AcTail>(P.obs, (uint32_t)p.n, (uint32_t)env, valid, lane, P.w1, P.w2, P.b2, P.rng,
                                              P.pairs, P.logits, (float)p.timestep[env], p.F, p.C, p.ksteps, nullptr,
                                              0, nullptr, &tail);
}

static_assert(FOLD_LOG2E == K_LOG2E && HIDDEN == OC_POLICY_HIDDEN, "oc_policy_layout.h restates these");

// The second layer as the packers are handed it: w2 [4 + C][64], b2 [4 + C] and, with a value head,
// wv [64], bv [1] in VALUE_ROW.  weights(o) / bias(o): those of row o of the second product, or NULL.
struct SecondLayer {
  const float *w2, *b2, *wv, *bv;
  int C;
  const float *weights(int o) const {
    const int lg = logit_of_row(o, C);
    return lg >= 0 ? w2 + (size_t)lg * HIDDEN : (o == VALUE_ROW && wv) ? wv : nullptr;
  }
  const float *bias(int o) const {
    const int lg = logit_of_row(o, C);
    return lg >= 0 ? b2 + lg : (o == VALUE_ROW && bv) ? bv : nullptr;
  }
};
void pack_second(const SecondLayer &L, uint16_t *out) {
  _Float16 *o = (_Float16 *)out;
  for (int el = 0; el < W2_ELEMS; el++) {
    const RowHid s = w2_source(el);
    const float *w = L.weights(s.row);
    o[el] = w ? fold(w[s.hid], FOLD_W2) : (_Float16)0.0f;
  }
}
void pack_second_start(const SecondLayer &L, float *out) {
  for (int el = 0; el < B2_ELEMS; el++) {
    const int row = b2_row(el);
    const float *w = L.weights(row);
    out[el] = w ? b2_start(*L.bias(row), w) : 0.0f;
  }
}
bool bad_comm(int32_t C) { return C < 1 || C > OC_POLICY_MAX_COMM; }

// ---- the one launcher of the two forward kernels ------------------------------------------------
// A kernel family: its argument struct and its instantiations.
struct Mlp {
  using Args = ::Args;
  template <int OT, int WPB, int CMAX>
  static constexpr auto kernel = k_policy_mlp<OT, WPB, CMAX>;
};
struct MlpAc {
  using Args = AcArgs;
  template <int OT, int WPB, int CMAX>
  static constexpr auto kernel = k_policy_mlp_ac<OT, WPB, CMAX>;
};
template <int N>
struct Int { static constexpr int value = N; };

template <class Fam>
auto dispatch(int obs_type, int C, int wpb) -> void (*)(const typename Fam::Args, int, int) {
  const auto by_wpb = [&](auto ot, auto cm) {
    constexpr int OT = decltype(ot)::value, CM = decltype(cm)::value;
    return wpb == 2 ? Fam::template kernel<OT, 2, CM> : Fam::template kernel<OT, 1, CM>;
  };
  const auto by_c = [&](auto ot) {
    return C <= 4 ? by_wpb(ot, Int<4>()) : C <= 8 ? by_wpb(ot, Int<8>()) : by_wpb(ot, Int<16>());
  };
  return obs_type == 1 ? by_c(Int<1>()) : obs_type == 2 ? by_c(Int<2>()) : by_c(Int<0>());
}

// Checks, grid and launch for entry point `who`.  need(player): what is wrong with one player, or
// NULL; the players are looked at before the n == 0 return (players_first) or behind the size checks.
template <class Fam, class Player, class Need>
int launch(const char *who, bool players_first, Need need, const Player *players, int32_t num_players,
           const double *timestep, int32_t F, int32_t C, int32_t obs_type, int64_t n, void *stream) {
  if (!players || num_players < 1 || num_players > 2 || !timestep || F < 1 || bad_comm(C) || obs_type < 0 ||
      obs_type > 2 || n < 0)
    return fail("%s: bad argument (1..2 players, 1 <= C <= 16, obs_type 0..2)", who);
  typename Fam::Args a;
  memset(&a, 0, sizeof(a));
  const auto take_players = [&]() {
    for (int k = 0; k < num_players; k++) {
      if (const char *why = need(players[k])) return fail("%s: %s", who, why);
      a.pl[k] = players[k];
    }
    return 0;
  };
  if (players_first && take_players() != 0) return -1;
  if (n == 0) return 0;
  if ((int64_t)F * n >= ((int64_t)1 << 31)) return fail("%s: F * n must stay below 2^31; split the batch", who);
  if (!players_first && take_players() != 0) return -1;
  a.timestep = timestep;
  a.F = F, a.C = C, a.ksteps = ksteps(F), a.n = n;
  const char *ev = getenv("OC_POLICY_WG32");   // tuning / A-B: 32-env workgroups in launch order
  const int wpb = (ev && ev[0] == '1') ? 1 : 2;
  const int64_t gx = (n + 32 * wpb - 1) / (32 * wpb), gx8 = (gx + 7) / 8 * 8;
  if (gx8 * num_players > 0x7FFFFFFF) return fail("%s: n too large", who);
  hipLaunchKernelGGL(dispatch<Fam>(obs_type, C, wpb), dim3((unsigned)(gx8 * num_players)), dim3(64 * wpb), 0,
                     (hipStream_t)stream, a, (int)gx, (int)gx8);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fail("%s: kernel launch: %s", who, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace

extern "C" {

int oc_policy_abi_version(void) { return OC_POLICY_ABI_VERSION; }
const char *oc_policy_last_error(void) { return g_err; }
int32_t oc_policy_ksteps(int32_t F) { return ksteps(F); }

int oc_policy_pack_w1(const float *w1, const float *wt, const float *b1, int32_t F, uint16_t *out) {
  if (!w1 || !wt || !b1 || !out || F < 1) return fail("oc_policy_pack_w1: bad argument");
  const int ks = ksteps(F);
  _Float16 *o = (_Float16 *)out;
  for (int el = 0; el < w1_elems(ks); el++) {
    const HidK s = w1_source(el, ks);
    const float v = s.k < F ? w1[(size_t)s.hid * F + s.k] : s.k == F ? wt[s.hid] : s.k == F + 1 ? b1[s.hid] : 0.0f;
    o[el] = fold(v, FOLD_W1);
  }
  return 0;
}

int oc_policy_pack_w2(const float *w2, int32_t C, uint16_t *out) {
  if (!w2 || !out || bad_comm(C)) return fail("oc_policy_pack_w2: bad argument (1 <= C <= 16)");
  pack_second({w2, nullptr, nullptr, nullptr, C}, out);
  return 0;
}

int oc_policy_pack_b2(const float *b2, const float *w2, int32_t C, float *out) {
  if (!b2 || !w2 || !out || bad_comm(C)) return fail("oc_policy_pack_b2: bad argument (1 <= C <= 16)");
  pack_second_start({w2, b2, nullptr, nullptr, C}, out);
  return 0;
}

// The value head rides in VALUE_ROW of the second product, folded exactly as a logit row is; every
// other element is oc_policy_pack_w2's / _b2's.
int oc_policy_pack_w2v(const float *w2, const float *wv, int32_t C, uint16_t *out) {
  if (!wv) return fail("oc_policy_pack_w2v: bad argument (wv)");
  if (!w2 || !out || bad_comm(C)) return fail("oc_policy_pack_w2: bad argument (1 <= C <= 16)");
  pack_second({w2, nullptr, wv, nullptr, C}, out);
  return 0;
}

int oc_policy_pack_b2v(const float *b2, const float *w2, const float *bv, const float *wv, int32_t C, float *out) {
  if (!bv || !wv) return fail("oc_policy_pack_b2v: bad argument (bv, wv)");
  if (!b2 || !w2 || !out || bad_comm(C)) return fail("oc_policy_pack_b2: bad argument (1 <= C <= 16)");
  pack_second_start({w2, b2, wv, bv, C}, out);
  return 0;
}

// the learner's image (include/oc_policy.h: w2t): the same folded values, fp32, in w2t_source's order
int oc_policy_pack_w2t(const float *w2, const float *wv, int32_t C, float *out) {
  if (!wv) return fail("oc_policy_pack_w2t: bad argument (wv)");
  if (!w2 || !out || bad_comm(C)) return fail("oc_policy_pack_w2t: bad argument (1 <= C <= 16)");
  const SecondLayer L = {w2, nullptr, wv, nullptr, C};
  for (int el = 0; el < W2T_ELEMS; el++) {
    const RowHid s = w2t_source(el);
    const float *w = L.weights(s.row);
    out[el] = w ? (float)fold(w[s.hid], FOLD_W2) : 0.0f;
  }
  return 0;
}

int oc_policy_mlp(const oc_policy_player *players, int32_t num_players, const double *timestep, int32_t F,
                  int32_t C, int32_t obs_type, int64_t n, void *stream) {
  const auto need = [](const oc_policy_player &p) -> const char * {
    return (!p.obs || !p.w1 || !p.w2 || !p.b2 || !p.pairs) ? "a player needs obs, w1, w2, b2 and pairs" : nullptr;
  };
  return launch<Mlp>("oc_policy_mlp", false, need, players, num_players, timestep, F, C, obs_type, n, stream);
}

int oc_policy_mlp_ac(const oc_policy_ac_player *players, int32_t num_players, const double *timestep, int32_t F,
                     int32_t C, int32_t obs_type, int64_t n, void *stream) {
  const auto need = [](const oc_policy_ac_player &p) -> const char * {
    if (!p.p.obs || !p.p.w1 || !p.p.w2 || !p.p.b2) return "a player needs obs, w1, w2 and b2";
    return (!p.move_row != !p.comm_row) ? "move_row and comm_row are given together" : nullptr;
  };
  return launch<MlpAc>("oc_policy_mlp_ac", true, need, players, num_players, timestep, F, C, obs_type, n, stream);
}

}  // extern "C"
