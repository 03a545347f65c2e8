// oc_policy_rppo.hip -- the recurrent PPO update's entry points of liboc_policy.so (include/oc_policy.h, last
// section but one: oc_policy_rppo_plan / _pack_bwd / _grad / _update); the kernels are in oc_policy_rppo_device.h,
// the checks, the plan and the launches in oc_policy_rppo_host.h (shared with oc_policy_rtrain.hip).  A
// translation unit and code object of its own, between the recurrent seat's and the train sequences': it holds
// the TRAIN = false kernels only, and the other units' kernels stay what they were.  gfx950 only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/oc_policy.h"
#include "oc_policy_fail.h"
#include "oc_policy_layout.h"
#include "oc_policy_rppo_device.h"
#include "oc_policy_rppo_host.h"

using namespace ocpol;

namespace {

int rppo_run(const char *who, const oc_rppo_cfg *c, const int32_t *envs, int32_t E, void *stream, bool apply) {
  if (rppo_check(who, c, envs, E, apply) != 0) return -1;
  return rppo_launch<false>(who, c, nullptr, envs, E, stream, apply);
}

}  // namespace

extern "C" {

int oc_policy_rppo_plan(int32_t F, int32_t C, int32_t T, int32_t E, int32_t max_groups, int64_t *plan) {
  if (!plan || rppo_bad_shape(F, C, T, E, max_groups))
    return fail("oc_policy_rppo_plan: bad argument (%s)", RPPO_SHAPE_RULE);
  rppo_make_plan(F, C, T, E, max_groups, plan);
  return 0;
}

int32_t oc_policy_rppo_pack_bwd_elems(void) { return LSTM_BWD_ELEMS; }

int oc_policy_rppo_pack_bwd(const float *wh, const float *w2, const float *wv, int32_t C, float *out) {
  if (!wh || !w2 || !wv || !out || C < 1 || C > OC_POLICY_MAX_COMM)
    return fail("oc_policy_rppo_pack_bwd: bad argument (1 <= C <= 16)");
  for (int el = 0; el < LSTM_WHT_ELEMS; el++) {
    const GateHid s = lstm_wht_source(el);
    const float w = wh[(size_t)(HIDDEN * s.gate + s.unit) * HIDDEN + s.hid];
    out[el] = (float)fold(w, lstm_gate_fold(s.gate)) * lstm_gate_unfold(s.gate);
  }
  for (int el = 0; el < W2T_ELEMS; el++) {
    const RowHid s = w2t_source(el);
    const int lg = logit_of_row(s.row, C);
    const float *w = lg >= 0 ? w2 + (size_t)lg * HIDDEN : s.row == VALUE_ROW ? wv : nullptr;
    out[LSTM_WHT_ELEMS + el] = w ? (float)fold(w[s.hid], FOLD_LOG2E) * FOLD_LN2 : 0.0f;
  }
  return 0;
}

int oc_policy_rppo_update(const oc_rppo_cfg *cfg, const int32_t *envs, int32_t E, void *stream) {
  return rppo_run("oc_policy_rppo_update", cfg, envs, E, stream, true);
}
int oc_policy_rppo_grad(const oc_rppo_cfg *cfg, const int32_t *envs, int32_t E, void *stream) {
  return rppo_run("oc_policy_rppo_grad", cfg, envs, E, stream, false);
}

}  // extern "C"
