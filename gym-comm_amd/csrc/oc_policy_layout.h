// oc_policy_layout.h -- where the policy's weights sit in the MFMA fragment images, stated once
// (the contract in prose: include/oc_policy.h; why the layouts are these: oc_policy_device.h).  Read
// by the host packers (oc_policy.hip), by the PPO kernels (oc_policy_ppo_device.h) and, alone, by a
// host compiler (tests/policy_layout_driver.cc): plain C++, no HIP header.
//
// Each image has a map from its element index to the logical coordinates the element takes its value
// from; an element whose coordinates name no weight (a feature past F + 1, a row no head uses) is
// padding and holds +0.
#ifndef OC_POLICY_LAYOUT_H
#define OC_POLICY_LAYOUT_H

#ifdef __HIP__
#define OC_HD __attribute__((host)) __attribute__((device))
#else
#define OC_HD
#endif

namespace ocpol {

constexpr int HIDDEN = 64;
constexpr int VALUE_ROW = 8;   // the value head's row of the second product: register 4 of the lower half-wave

// 16-feature k-steps of the first product: F observation rows, the timestep, the constant 1
OC_HD constexpr int ksteps(int F) { return (F + 2 + 15) / 16; }

// the row of a 32-row product that accumulator register q of half-wave h holds
OC_HD constexpr int acc_row(int q, int h) { return (q & 3) + 8 * (q >> 2) + 4 * h; }

// which logit (0..3 move, 4 + c comm) lives in row o of the second product, or -1
OC_HD constexpr int logit_of_row(int o, int C) {
  if (o < 4) return o;
  if (((o - 4) & 7) < 4) {
    const int c = ((o - 4) & 3) + 4 * ((o - 4) >> 3);
    if (c < C) return 4 + c;
  }
  return -1;
}

struct HidK { int hid, k; };     // hidden unit, augmented feature (k < F: W1, F: wt, F + 1: b1, else none)
struct RowHid { int row, hid; }; // row of the second product (a logit's, VALUE_ROW, else none), hidden unit

// w1 fp16 [2][ks][64][8]: element j of lane l, M-tile m, k-step s
OC_HD constexpr int w1_elems(int ks) { return 2 * ks * 64 * 8; }
OC_HD constexpr HidK w1_source(int el, int ks) {
  const int j = el & 7, l = (el >> 3) & 63, s = (el >> 9) % ks, m = (el >> 9) / ks;
  return {32 * m + (l & 31), 16 * s + 8 * (l >> 5) + j};
}
// w2 fp16 [4][64][8]: element j of lane l, k-step s; k permuted to the first product's accumulator order
constexpr int W2_ELEMS = 4 * 64 * 8;
OC_HD constexpr RowHid w2_source(int el) {
  const int j = el & 7, l = (el >> 3) & 63, s = el >> 9;
  return {l & 31, 16 * s + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)};
}
// b2 fp32 [64][16]: register q of lane l starts at its row's value
constexpr int B2_ELEMS = 64 * 16;
OC_HD constexpr int b2_row(int el) { return acc_row(el & 15, el >> 9); }
// w2t fp32 [2][16][64]: lane l of k-step t, M-tile m -- W2 transposed, k in the order of d logits
constexpr int W2T_ELEMS = 2 * 16 * 64;
OC_HD constexpr RowHid w2t_source(int el) {
  const int l = el & 63, t = (el >> 6) & 15, m = el >> 10;
  return {acc_row(t, l >> 5), 32 * m + (l & 31)};
}

// offsets of the seven tensors in the flat parameter vector [P], and where a fragment's logical
// coordinates land in it (-1: none)
struct PpoLayout {
  int F, C, wt, b1, w2, b2, wv, bv, P;
  OC_HD constexpr PpoLayout(int F_, int C_)
      : F(F_), C(C_), wt(64 * F_), b1(wt + 64), w2(b1 + 64), b2(w2 + (4 + C_) * 64), wv(b2 + 4 + C_), bv(wv + 64),
        P(bv + 1) {}
  OC_HD constexpr int first(int hid, int k) const {
    return k < F ? hid * F + k : k == F ? wt + hid : k == F + 1 ? b1 + hid : -1;
  }
  OC_HD constexpr int second(int row, int hid) const {
    const int lg = logit_of_row(row, C);
    return lg >= 0 ? w2 + lg * 64 + hid : row == VALUE_ROW ? wv + hid : -1;
  }
  OC_HD constexpr int bias(int row) const {
    const int lg = logit_of_row(row, C);
    return lg >= 0 ? b2 + lg : row == VALUE_ROW ? bv : -1;
  }
};

// ---- the recurrent seat (include/oc_policy.h, its own section; oc_policy_lstm.hip) -----------------
// gates fp16 [4 gates][2][ks][64][8], gates in the order i, f, g, o: element j of lane l, M-tile (gate, m),
// k-step s of ks = ksteps(F) + LSTM_HSTEPS.  Tile (gate, m) holds rows 64 gate + 32 m .. + 31 of the 256,
// i.e. units 32 m .. 32 m + 31: the four gates of a unit share a lane and an accumulator register.  The
// x k-steps come first (k as in w1: < F Wx, F wt, F + 1 b); behind them the four k-steps over h, k
// permuted to the accumulator order as w2's is (k = -1, hid = the column of Wh).
constexpr int LSTM_GATES = 4, LSTM_HSTEPS = 4;
enum { LSTM_I = 0, LSTM_F = 1, LSTM_G = 2, LSTM_O = 3 };
OC_HD constexpr int lstm_ksteps(int F) { return ksteps(F) + LSTM_HSTEPS; }
OC_HD constexpr int lstm_gate_elems(int F) { return LSTM_GATES * 2 * lstm_ksteps(F) * 64 * 8; }
struct GateSrc { int gate, unit, k, hid; };   // row 64 gate + unit of the 256; k >= 0: an x column; else column hid of Wh
OC_HD constexpr GateSrc lstm_gate_source(int el, int F) {
  const int ks = lstm_ksteps(F), kx = ksteps(F);
  const int j = el & 7, l = (el >> 3) & 63, s = (el >> 9) % ks, t = (el >> 9) / ks;
  const int unit = 32 * (t & 1) + (l & 31);
  return s < kx ? GateSrc{t >> 1, unit, 16 * s + 8 * (l >> 5) + j, -1}
                : GateSrc{t >> 1, unit, -1, 16 * (s - kx) + 8 * (j >> 2) + 4 * (l >> 5) + (j & 3)};
}
// the head images are w2's and b2's maps (w2_source, b2_row) with other values: log2(e) [W2; wv] and
// log2(e) [b2; bv], no row-sum fold (the product takes h itself)

// ---- the recurrent update (include/oc_policy.h, last section; oc_policy_rppo.hip) -------------------
// offsets of the eight tensors in the flat parameter vector [P], and where a product's logical
// coordinates land in it (-1: none): row = 64 gate + unit of the 256 gate rows
struct RppoLayout {
  int F, C, wt, b, wh, w2, b2, wv, bv, P;
  OC_HD constexpr RppoLayout(int F_, int C_)
      : F(F_), C(C_), wt(256 * F_), b(wt + 256), wh(b + 256), w2(wh + 256 * HIDDEN), b2(w2 + (4 + C_) * 64),
        wv(b2 + 4 + C_), bv(wv + 64), P(bv + 1) {}
  OC_HD constexpr int gate(int row, int k) const {
    return k < 0 ? -1 : k < F ? row * F + k : k == F ? wt + row : k == F + 1 ? b + row : -1;
  }
  OC_HD constexpr int rec(int row, int hid) const { return wh + row * HIDDEN + hid; }
  OC_HD constexpr int second(int row, int hid) const {
    const int lg = logit_of_row(row, C);
    return lg >= 0 ? w2 + lg * 64 + hid : row == VALUE_ROW ? wv + hid : -1;
  }
  OC_HD constexpr int bias(int row) const {
    const int lg = logit_of_row(row, C);
    return lg >= 0 ? b2 + lg : row == VALUE_ROW ? bv : -1;
  }
};
// the backward's image, fp32 [LSTM_BWD_ELEMS]: first wht [2][8][16][64] -- lane l of k-step (tile, q), M-tile
// m: Wh transposed, k in the order in which d z sits in the gate product's accumulators (register q of tile
// (gate, mm) = row 64 gate + 32 mm + acc_row(q, l >> 5)), hidden unit 32 m + (l & 31) -- then the head's
// w2t [2][16][64] through w2t_source.  The values are those of the network the fp16 images represent: the
// folded fp16 weight times the inverse of its fold (lstm_gate_unfold; ln 2 for the head).
constexpr int LSTM_WHT_ELEMS = 2 * 8 * 16 * 64;
constexpr int LSTM_BWD_ELEMS = LSTM_WHT_ELEMS + W2T_ELEMS;
struct GateHid { int gate, unit, hid; };   // row 64 gate + unit of Wh, column hid
OC_HD constexpr GateHid lstm_wht_source(int el) {
  const int l = el & 63, q = (el >> 6) & 15, t = (el >> 10) & 7, m = el >> 13;
  return {t >> 1, 32 * (t & 1) + acc_row(q, l >> 5), 32 * m + (l & 31)};
}

// ---- the values: the activation's constants folded in (oc_policy_device.h: sigmoid_complement) ----
#ifdef __FLT16_MAX__   // (a host compiler without _Float16 still gets the maps above)
constexpr float FOLD_LOG2E = 1.4426950408889634f;
constexpr float FOLD_W1 = 2.0f * FOLD_LOG2E, FOLD_W2 = -2.0f * FOLD_LOG2E;
// the recurrent seat's gates: sigmoid(z) = sigmoid_complement(-log2(e) z), tanh(z) = 1 - 2 sigmoid_complement(2 log2(e) z)
OC_HD constexpr float lstm_gate_fold(int gate) { return gate == LSTM_G ? FOLD_W1 : -FOLD_LOG2E; }
// the inverse folds, as the recurrent update's backward image multiplies by them (one fp32 product)
constexpr float FOLD_LN2 = 0.6931471805599453f;
OC_HD constexpr float lstm_gate_unfold(int gate) { return gate == LSTM_G ? 0.5f * FOLD_LN2 : -FOLD_LN2; }

// the fp16 value a product multiplies by: the product in fp32, rounded once
OC_HD inline _Float16 fold(float w, float scale) { return (_Float16)(scale * w); }

// b2's element for a row with bias b and weights wrow [64]: log2(e) (b + sum_j W[j]) with the sum taken
// over the ROUNDED folded weights, j ascending, so that the fold is exact
OC_HD inline float b2_start(float b, const float *wrow) {
#pragma clang fp contract(off)
  float sum = 0.0f;
  for (int j = 0; j < HIDDEN; j++) sum += (float)fold(wrow[j], FOLD_W2);
  return FOLD_LOG2E * b - 0.5f * sum;
}
#endif

}  // namespace ocpol
#endif
