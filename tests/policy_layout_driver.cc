// policy_layout_driver.cc -- gym-comm_amd/csrc/oc_policy_layout.h alone, by a host compiler under the
// address and undefined-behaviour sanitizers (tests/test_policy_layout_cpu.py): every map of the
// fragment layout is checked exhaustively to be the bijection the kernels rely on.
#include <stdio.h>

#include <vector>

#include "../gym-comm_amd/csrc/oc_policy_layout.h"

using namespace ocpol;

static int failures = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      failures++;                                \
      printf("FAILED %s: ", #cond);              \
      printf(__VA_ARGS__);                       \
      printf("\n");                              \
    }                                            \
  } while (0)

int main() {
  // the accumulator row: (q, h) -> 0..31, one-to-one
  {
    std::vector<int> seen(32, 0);
    for (int h = 0; h < 2; h++)
      for (int q = 0; q < 16; q++) {
        const int row = acc_row(q, h);
        CHECK(row >= 0 && row < 32, "q %d h %d", q, h);
        seen[row]++;
      }
    for (int row = 0; row < 32; row++) CHECK(seen[row] == 1, "row %d", row);
    CHECK(acc_row(4, 0) == VALUE_ROW, "the value head is register 4 of the lower half-wave");
  }
  const int Fs[] = {1, 14, 15, 30, 46, 62};
  for (int C = 1; C <= 16; C++) {
    // logit_of_row: exactly 4 + C rows, one-to-one onto 0 .. 3 + C, never the value row
    std::vector<int> row_of(4 + C, -1);
    int live = 0;
    for (int o = 0; o < 32; o++) {
      const int lg = logit_of_row(o, C);
      if (lg < 0) continue;
      live++;
      CHECK(lg < 4 + C && row_of[lg] == -1, "C %d row %d logit %d", C, o, lg);
      CHECK(o != VALUE_ROW, "C %d", C);
      if (lg < 4 + C) row_of[lg] = o;
    }
    CHECK(live == 4 + C, "C %d: %d rows", C, live);
    std::vector<int> is_live(32, 0);   // the rows a head uses: the logits' and the value head's
    for (int lg = 0; lg < 4 + C; lg++)
      if (row_of[lg] >= 0) is_live[row_of[lg]] = 1;
    is_live[VALUE_ROW] = 1;

    // w2, w2t: every (live row, hidden) is the source of exactly one element; b2: 32 elements per row
    std::vector<int> n2(32 * HIDDEN, 0), nt(32 * HIDDEN, 0), nb(32, 0);
    for (int el = 0; el < W2_ELEMS; el++) {
      const RowHid s = w2_source(el);
      CHECK(s.row >= 0 && s.row < 32 && s.hid >= 0 && s.hid < HIDDEN, "w2 element %d", el);
      n2[s.row * HIDDEN + s.hid]++;
    }
    for (int el = 0; el < W2T_ELEMS; el++) {
      const RowHid s = w2t_source(el);
      CHECK(s.row >= 0 && s.row < 32 && s.hid >= 0 && s.hid < HIDDEN, "w2t element %d", el);
      nt[s.row * HIDDEN + s.hid]++;
    }
    for (int el = 0; el < B2_ELEMS; el++) {
      const int row = b2_row(el);
      CHECK(row >= 0 && row < 32, "b2 element %d", el);
      nb[row]++;
    }
    for (int row = 0; row < 32; row++)
      if (is_live[row]) {
        for (int hid = 0; hid < HIDDEN; hid++)
          CHECK(n2[row * HIDDEN + hid] == 1 && nt[row * HIDDEN + hid] == 1, "C %d row %d hidden %d", C, row, hid);
        CHECK(nb[row] == 32, "C %d row %d: %d b2 elements", C, row, nb[row]);
      }

    for (int F : Fs) {
      const int ks = ksteps(F);
      CHECK(16 * ks >= F + 2 && 16 * (ks - 1) < F + 2, "F %d ksteps %d", F, ks);
      // w1: every (hidden, k < F + 2) is the source of exactly one element, every other element has none
      std::vector<int> n1(HIDDEN * (F + 2), 0);
      const PpoLayout lay(F, C);
      for (int el = 0; el < w1_elems(ks); el++) {
        const HidK s = w1_source(el, ks);
        CHECK(s.hid >= 0 && s.hid < HIDDEN && s.k >= 0 && s.k < 16 * ks, "w1 element %d F %d", el, F);
        if (s.k < F + 2) n1[s.hid * (F + 2) + s.k]++;
        CHECK((lay.first(s.hid, s.k) >= 0) == (s.k < F + 2), "w1 element %d F %d", el, F);
      }
      for (int i = 0; i < HIDDEN * (F + 2); i++) CHECK(n1[i] == 1, "F %d hidden %d k %d", F, i / (F + 2), i % (F + 2));

      // PpoLayout: the seven ranges partition [0, P), and the three lookups reach every index once
      const int starts[8] = {0, lay.wt, lay.b1, lay.w2, lay.b2, lay.wv, lay.bv, lay.P};
      const int sizes[7] = {HIDDEN * F, HIDDEN, HIDDEN, (4 + C) * HIDDEN, 4 + C, HIDDEN, 1};
      for (int t = 0; t < 7; t++) CHECK(starts[t + 1] - starts[t] == sizes[t], "F %d C %d tensor %d", F, C, t);
      std::vector<int> np(lay.P, 0);
      const auto count = [&](int pi, int lo, int hi) {
        CHECK(pi >= lo && pi < hi, "F %d C %d index %d outside [%d, %d)", F, C, pi, lo, hi);
        if (pi >= 0 && pi < lay.P) np[pi]++;
      };
      for (int hid = 0; hid < HIDDEN; hid++)
        for (int k = 0; k < 16 * ks; k++)
          if (k < F + 2) count(lay.first(hid, k), starts[k < F ? 0 : k == F ? 1 : 2], starts[k < F ? 1 : k == F ? 2 : 3]);
          else CHECK(lay.first(hid, k) == -1, "F %d k %d", F, k);
      for (int row = 0; row < 32; row++) {
        const bool value = row == VALUE_ROW;
        if (!is_live[row]) {
          CHECK(lay.bias(row) == -1 && lay.second(row, 0) == -1 && lay.second(row, HIDDEN - 1) == -1, "row %d", row);
          continue;
        }
        count(lay.bias(row), starts[value ? 6 : 4], starts[value ? 7 : 5]);
        for (int hid = 0; hid < HIDDEN; hid++) count(lay.second(row, hid), starts[value ? 5 : 3], starts[value ? 6 : 4]);
      }
      for (int pi = 0; pi < lay.P; pi++) CHECK(np[pi] == 1, "F %d C %d parameter %d reached %d times", F, C, pi, np[pi]);
    }
  }
  printf("failures: %d\n", failures);
  return failures != 0;
}
