// oc_policy_lstm.hip -- the recurrent seat of liboc_policy.so (include/oc_policy.h, last section): one
// LSTM cell of 64 units, the actor's and the critic's heads on its output and the actor-critic tail
// (oc_policy_ac_device.h: AcTail, as it is), in ONE launch.  A translation unit and code object of its
// own, between the update's and the train sequence's: the other units' kernels stay what they were.
//
// gfx950 only.  One wave = 32 envs, two waves per workgroup, workgroup x = envs 64 x .. 64 x + 63 (the
// step kernels' mapping).  Per wave:
//
//   Z^T [256 gate rows x 32 envs] = [Wx | wt | b | Wh]' . [x; ts; 1; h_in]     v_mfma_f32_32x32x16_f16
//       8 M-tiles (gate, m) of 32 rows, 8 x 16 accumulator registers; the x k-steps form their B operand
//       as policy_pass does, the four k-steps over h take the stored state in the accumulator order
//       (lane (env, half) holds units 16 s + 8 (j >> 2) + 4 half + (j & 3)): the A fragments' k index is
//       permuted on the host instead.  Register q of tile (gate, m) is gate `gate` of unit
//       32 m + acc_row(q, half) of the lane's env, so
//   the cell update is lane-local: 32 units per lane, each from four registers and one c_in, and
//   h comes out where a product over the units wants its B operand: registers 8 (s & 1) .. + 7 of tile
//       s >> 1 are the fragment of k-step s of the head product -- and of the next step's product over h,
//       which is why a lane reads exactly the state elements it writes.
//
// The A fragments (8 tiles x ks k-steps x 1 KiB, 57 KiB at ks = 7) are streamed from L2 by every wave;
// nothing is staged in LDS, nothing spills.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "../../include/oc_policy.h"
#include "oc_policy_device.h"
#include "oc_policy_ac_device.h"
#include "oc_policy_fail.h"
#include "oc_policy_layout.h"

namespace {

using namespace ocpol;

struct LstmArgs {
  oc_policy_lstm_player pl;
  const double *timestep;
  int32_t F, C, kx;      // kx: the k-steps over x (ksteps(F))
  int64_t n;
};

constexpr float K_TANH = 2.0f * K_LOG2E;   // tanh(c) = 1 - 2 r(K_TANH * c)

template <int OT, int CMAX>
__global__ void __launch_bounds__(128) k_policy_lstm(const LstmArgs p) {
  const oc_policy_lstm_player &P = p.pl;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int64_t env0 = ((int64_t)blockIdx.x * 2 + (threadIdx.x >> 6)) * 32 + r;
  const bool valid = env0 < p.n;
  // lanes past the batch compute on the last env and store nothing
  const uint32_t env = (uint32_t)(valid ? env0 : p.n - 1), n32 = (uint32_t)p.n;
  const int F = p.F, kx = p.kx, ks = kx + LSTM_HSTEPS;
  const float ts = (float)p.timestep[env];
  const bool start = P.episode_start != nullptr && P.episode_start[env] > 0.0f;
  const half8 *wg = (const half8 *)P.gates + lane;

  // this lane's state: unit 32 m + acc_row(q, h) in [m][q] -- every element it will write, read first
  float hin[2][16], cin[2][16];
#pragma unroll
  for (int m = 0; m < 2; m++)
#pragma unroll
    for (int q = 0; q < 16; q++) {
      const uint32_t at = (uint32_t)(32 * m + acc_row(q, h)) * n32 + env;
      const float hv = P.h_in[at], cv = P.c_in[at];
      hin[m][q] = start ? 0.0f : hv;   // a select: whatever the old state held is gone
      cin[m][q] = start ? 0.0f : cv;
    }

  f32x16 acc[8];   // tile t = 2 gate + m
#pragma unroll
  for (int t = 0; t < 8; t++)
#pragma unroll
    for (int q = 0; q < 16; q++) acc[t][q] = 0.0f;

  // ---- the k-steps over x: policy_pass's B operand (oc_policy_device.h) ------------------------------
  for (int s = 0; s < kx; s++) {
    half8 b;
    const uint32_t k0 = 16 * s + 8 * h, off0 = k0 * n32 + env;
    if (16 * s + 16 <= F) {   // uniform: every feature of this k-step is an observation row
#pragma unroll
      for (int j = 0; j < 8; j++) b[j] = (_Float16)obs_at<OT>(P.obs, off0 + (uint32_t)j * n32);
    } else {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int k = (int)k0 + j;
        const float xv = obs_at<OT>(P.obs, k < F ? off0 + (uint32_t)j * n32 : env);   // (always a readable element)
        b[j] = (_Float16)(k < F ? xv : k == F ? ts : k == F + 1 ? 1.0f : 0.0f);
      }
    }
#pragma unroll
    for (int t = 0; t < 8; t++)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg[(size_t)(t * ks + s) * 64], b, acc[t], 0, 0, 0);
  }
  // ---- the four over h: registers 8 (s & 1) .. + 7 of the state's tile s >> 1 --------------------------
#pragma unroll
  for (int s = 0; s < LSTM_HSTEPS; s++) {
    half8 b;
#pragma unroll
    for (int j = 0; j < 8; j++) b[j] = (_Float16)hin[s >> 1][8 * (s & 1) + j];
#pragma unroll
    for (int t = 0; t < 8; t++)
      acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wg[(size_t)(t * ks + kx + s) * 64], b, acc[t], 0, 0, 0);
  }

  // ---- the cell, lane-local; h straight into the head product's B operand ------------------------------
  f32x16 out;
  {
    const float4 *hb = (const float4 *)P.head_bias + lane * 4;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const float4 v = hb[q];
      out[4 * q + 0] = v.x, out[4 * q + 1] = v.y, out[4 * q + 2] = v.z, out[4 * q + 3] = v.w;
    }
  }
  half8 wh[4];   // (loaded in front of the state's stores, which the compiler must take for possible aliases)
#pragma unroll
  for (int s = 0; s < 4; s++) wh[s] = ((const half8 *)P.head)[s * 64 + lane];
#pragma unroll
  for (int s = 0; s < 4; s++) {
    const int m = s >> 1;
    half8 b;
#pragma unroll
    for (int j = 0; j < 8; j++) {
#pragma clang fp contract(off)
      const int q = 8 * (s & 1) + j;
      const float gi = sigmoid_complement(acc[2 * LSTM_I + m][q]);
      const float gf = sigmoid_complement(acc[2 * LSTM_F + m][q]);
      const float gg = 1.0f - 2.0f * sigmoid_complement(acc[2 * LSTM_G + m][q]);
      const float go = sigmoid_complement(acc[2 * LSTM_O + m][q]);
      const float keep = gf * cin[m][q], add = gi * gg;
      const float c = keep + add;
      const float hv = go * (1.0f - 2.0f * sigmoid_complement(K_TANH * c));
      const uint32_t at = (uint32_t)(32 * m + acc_row(q, h)) * n32 + env;
      if (valid && P.c_out != nullptr) P.c_out[at] = c;
      if (valid && P.h_out != nullptr) P.h_out[at] = hv;
      b[j] = (_Float16)hv;
    }
    out = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[s], b, out, 0, 0, 0);
  }

  const AcTail tail = {P.given, P.move_row, P.comm_row, P.log_prob, P.value};
  tail.template run<CMAX>(out, n32, env, valid, lane, P.rng, P.pairs, P.logits, p.C);
}

template <int OT>
auto by_comm(int C) -> void (*)(const LstmArgs) {
  return C <= 4 ? k_policy_lstm<OT, 4> : C <= 8 ? k_policy_lstm<OT, 8> : k_policy_lstm<OT, 16>;
}

bool bad_comm(int32_t C) { return C < 1 || C > OC_POLICY_MAX_COMM; }
bool bad_rows(int32_t F) { return F < 1 || F + 2 > 64; }

// rows of the head product as the packers are handed them: a logit's, the value's (VALUE_ROW), or NULL
const float *head_row(const float *w2, const float *wv, int C, int row, int stride) {
  const int lg = logit_of_row(row, C);
  return lg >= 0 ? w2 + (size_t)lg * stride : row == VALUE_ROW ? wv : nullptr;
}

}  // namespace

extern "C" {

int32_t oc_policy_lstm_ksteps(int32_t F) { return lstm_ksteps(F); }

int oc_policy_lstm_pack_gates(const float *wx, const float *wt, const float *b, const float *wh, int32_t F,
                              uint16_t *out) {
  if (!wx || !wt || !b || !wh || !out || bad_rows(F))
    return fail("oc_policy_lstm_pack_gates: bad argument (F >= 1, F + 2 <= 64)");
  _Float16 *o = (_Float16 *)out;
  for (int el = 0; el < lstm_gate_elems(F); el++) {
    const GateSrc s = lstm_gate_source(el, F);
    const int row = HIDDEN * s.gate + s.unit;
    const float v = s.k < 0       ? wh[(size_t)row * HIDDEN + s.hid]
                    : s.k < F     ? wx[(size_t)row * F + s.k]
                    : s.k == F    ? wt[row]
                    : s.k == F + 1 ? b[row]
                                   : 0.0f;
    o[el] = fold(v, lstm_gate_fold(s.gate));
  }
  return 0;
}

int oc_policy_lstm_pack_head(const float *w2, const float *wv, int32_t C, uint16_t *out) {
  if (!w2 || !wv || !out || bad_comm(C)) return fail("oc_policy_lstm_pack_head: bad argument (1 <= C <= 16)");
  _Float16 *o = (_Float16 *)out;
  for (int el = 0; el < W2_ELEMS; el++) {
    const RowHid s = w2_source(el);
    const float *w = head_row(w2, wv, C, s.row, HIDDEN);
    o[el] = w ? fold(w[s.hid], FOLD_LOG2E) : (_Float16)0.0f;
  }
  return 0;
}

int oc_policy_lstm_pack_head_bias(const float *b2, const float *bv, int32_t C, float *out) {
  if (!b2 || !bv || !out || bad_comm(C)) return fail("oc_policy_lstm_pack_head_bias: bad argument (1 <= C <= 16)");
  for (int el = 0; el < B2_ELEMS; el++) {
    const float *w = head_row(b2, bv, C, b2_row(el), 1);
    out[el] = w ? FOLD_LOG2E * *w : 0.0f;
  }
  return 0;
}

int oc_policy_lstm_ac(const oc_policy_lstm_player *pl, const double *timestep, int32_t F, int32_t C,
                      int32_t obs_type, int64_t n, void *stream) {
  if (!pl || !timestep || bad_rows(F) || bad_comm(C) || obs_type < 0 || obs_type > 2 || n < 0)
    return fail("oc_policy_lstm_ac: bad argument (F >= 1, F + 2 <= 64, 1 <= C <= 16, obs_type 0..2, n >= 0)");
  if (!pl->obs || !pl->gates || !pl->head || !pl->head_bias || !pl->h_in || !pl->c_in)
    return fail("oc_policy_lstm_ac: the player needs obs, gates, head, head_bias, h_in and c_in");
  if (!pl->move_row != !pl->comm_row) return fail("oc_policy_lstm_ac: move_row and comm_row are given together");
  if (n == 0) return 0;
  if ((int64_t)HIDDEN * n >= ((int64_t)1 << 31))
    return fail("oc_policy_lstm_ac: 64 n must stay below 2^31; split the batch");
  LstmArgs a;
  memset(&a, 0, sizeof(a));
  a.pl = *pl;
  a.timestep = timestep;
  a.F = F, a.C = C, a.kx = ksteps(F), a.n = n;
  const auto kernel = obs_type == 1 ? by_comm<1>(C) : obs_type == 2 ? by_comm<2>(C) : by_comm<0>(C);
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 63) / 64)), dim3(128), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    fail("oc_policy_lstm_ac: kernel launch: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // extern "C"
