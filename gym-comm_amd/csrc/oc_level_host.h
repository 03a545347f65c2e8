// oc_level_host.h -- the host half of a level: the uniform per-level header the kernels read
// (LevelHdr, RunCfg), the compiler from a level blob (include/oc_level.h) to that header, the text
// of a specialised library's header (oc_level_spec_source) and the host image of the device tables.
// Plain C++17: no GPU header, no GPU attribute -- tests/host_header_driver.cc compiles it with the
// host compiler under the address and undefined-behaviour sanitizers.  The library's one
// translation unit includes it first; oc_step_device.h holds the kernels that read what is built here.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/oc_level.h"
namespace {

constexpr int MAX_GOALS = 16;   // distinct goal type-sets (all 15 non-empty subsets of 4 types fit)
constexpr int MAX_DELS = 4;     // Deliver subtasks
constexpr int MAX_PAIRLK = 12;  // item-pair distance lookups of the shaping pair term
constexpr int MAX_NAMES = 16;   // dup mode: distinct merged names (4 bits of key rank each, two state words)

// Uniform per-level data.  Generic build: passed by value in the kernel arguments
// (scalar loads).  Specialised build (-DOC_SPECIALIZED, one .so per level, see
// gym-comm_amd/specialize.py): a constexpr object, so every loop bound, type test and
// bit-plane below folds at compile time and the kernels become straight-line code.
//
// ONE list of its fields, in declaration order: FLD / ARR(type, name[, extent]) are STRUCTURE, what
// the recipes and the item multiset fix; GFLD / GARR are GEOMETRY, the map itself (see the accessor
// classes in oc_step_device.h).  The struct, the kernels' accessors, the text of OC_SPEC_HDR and
// structure_of() are all generated from it, so they cannot disagree.
#define OC_HDR_FIELDS(FLD, ARR, GFLD, GARR)                                                          \
  GFLD(int32_t, W) GFLD(int32_t, H) GFLD(int32_t, ncells) GFLD(int32_t, max_path)                    \
  FLD(int32_t, S) FLD(int32_t, A) FLD(int32_t, M)                                                    \
  FLD(uint32_t, item_types)              /* nibble i = content type of item i */                     \
  GARR(uint64_t, nonfloor, 2)            /* bit c: cell c (= y*W + x) is not Floor */                \
  GARR(uint64_t, cell_lo, 2) GARR(uint64_t, cell_hi, 2)   /* cell type bit-planes */                 \
  FLD(uint32_t, nondeliver_mask) FLD(uint32_t, deliver_mask)   /* subtask bitmasks by kind */         \
  ARR(uint32_t, chop_mask, 3)            /* per food type: Chop(food) subtasks */                    \
  ARR(uint32_t, food_item, 3)            /* per food type: index of its item (255 = absent) */       \
  FLD(uint32_t, ngoal)                                                                               \
  ARR(uint32_t, goal_tset, MAX_GOALS)    /* distinct goal type-sets (bit t = type t present) */      \
  ARR(uint32_t, goal_nd, MAX_GOALS)      /* Chop/Merge subtasks whose goal is that set */            \
  ARR(uint32_t, goal_dl, MAX_GOALS)      /* Deliver subtasks whose goal is that set */               \
  FLD(uint32_t, ndel)                                                                                \
  ARR(uint32_t, del_tset, MAX_DELS) ARR(uint32_t, del_bit, MAX_DELS)   /* Deliver subtasks in subtask order */ \
  FLD(uint32_t, npairlk)                                                                             \
  ARR(uint32_t, pairlk, MAX_PAIRLK)      /* i | j<<4 | last_of_group<<8 */                           \
  FLD(uint32_t, pair_static_max)         /* name pairs with an absent type: each appends MAX_PATH */ \
  FLD(uint32_t, ndeliv)                                                                              \
  GARR(uint32_t, deliv_pos, OC_MAX_DELIV)   /* x | y<<4, world order */                              \
  GARR(int32_t, init_words, OC_MAX_AGENTS + OC_MAX_ITEMS + 4)                                        \
  GFLD(uint32_t, nquot)                  /* entries in the quotient table */                         \
  /* random-* levels: items placed on random Counter tiles at every reset */                         \
  FLD(uint32_t, nscatter) GFLD(uint32_t, ncounters)                                                  \
  ARR(uint32_t, scatter_item, 4)         /* world-order item id of each scattered letter, file order */ \
  /* levels that repeat a content type ("dup" mode; no built-in level does): an Object is then a      \
     MULTISET of types, and the kernels are instantiated with DUP = true */                          \
  FLD(uint32_t, has_dup)                                                                             \
  ARR(uint32_t, goal_sig, MAX_GOALS)     /* per distinct goal: its content counts (sig7: T | L<<2 | O<<4 | P<<6) */ \
  ARR(uint32_t, del_sig, MAX_DELS)       /* the same for the Deliver subtasks, subtask order */      \
  ARR(uint32_t, food_items, 3)           /* per food type: bit i = item i is of that type */         \
  FLD(uint32_t, nnames)                  /* merged names (multisets with >= 2 contents) a merge can create */ \
  ARR(uint32_t, name_sig, MAX_NAMES)                                                                 \
  /* two facts about the MAP that select code paths at compile time in a specialised build */        \
  FLD(uint32_t, closed_border)           /* every border cell is a non-Floor tile (see OC_BORDER_CLOSED) */ \
  FLD(uint32_t, planes128)               /* more than 64 cells: the tile bit-planes need both 64-bit words */

struct LevelHdr {
#define OC_F(T, name) T name;
#define OC_A(T, name, N) T name[N];
  OC_HDR_FIELDS(OC_F, OC_A, OC_F, OC_A)
#undef OC_F
#undef OC_A
};

// per-run settings that do not select a specialisation
struct RunCfg {
  int32_t T;          // arglist.max_num_timesteps (0 = no limit)
  uint32_t allergic;  // bit a: agent a is ALLERGIC
  double inv_T;       // 1.0 / T, correctly rounded on the host (0 when T == 0)
  double inv_max_path;  // 1.0 / MAX_PATH, correctly rounded on the host
  // The caller's subtask order is run-time data too.  Inside the kernels subtask bits sit in a
  // CANONICAL order (Chop / Merge subtasks sorted by kind, goal object and food; Deliver subtasks
  // after them in the caller's order, which the fp64 shaping sum follows), so one specialised
  // library serves every order of a level -- the reference's own order is `set` iteration order
  // and changes with PYTHONHASHSEED (recipe_planner/stripsworld.py:72-77).  slot4: byte s = the
  // bit of the caller's subtask s; only the completed_subtasks observation rows need it.
  uint32_t slot_identity;
  uint32_t slot4[OC_MAX_SUBTASKS / 4];
  uint32_t play;   // arglist.play: the "playable" branches of interact() (utils/interact.py:44-47,52,66-67)
};

// Every border cell of the map is a non-Floor tile: agents (always on Floor) can then never
// propose a cell outside the map, so the proposal needs no bounds test, no clamp and no
// OC_ERR_OOB path.  True for all fixed levels of the reference; decided at compile time in a
// per-level specialised build, never assumed by the generic library.
constexpr bool border_closed(const LevelHdr &L) {
  for (int y = 0; y < L.H; y++)
    for (int x = 0; x < L.W; x++)
      if (x == 0 || y == 0 || x == L.W - 1 || y == L.H - 1) {
        const int c = y * L.W + x;
        if (!((L.nonfloor[c >> 6] >> (c & 63)) & 1)) return false;
      }
  return true;
}

// the unit of content type t in an item word's Object signature: a bit of the type set, or (dup
// mode) the low bit of the type's two-bit count (oc_step_device.h: sig_of_type, checked there)
constexpr int item_sig_bit(bool dup, int t) { return 1 << (24 + (dup ? 2 : 1) * t); }

int tset_of_sig(int sig) {
  int ts = 0;
  for (int t = 0; t < OC_NTYPES; t++)
    if ((sig >> (4 * t)) & 15) ts |= 1 << t;
  return ts;
}
// nibble counts (include/oc_level.h goal_sig) -> the 7-bit form the dup-mode item words carry
// (two bits per food type, bit 6 the Plate); -1 when a count does not fit
int sig7_of_sig(int sig) {
  int out = 0;
  for (int t = 0; t < OC_NTYPES; t++) {
    const int c = (sig >> (4 * t)) & 15;
    if (c > (t == OC_PLATE ? 1 : 3)) return -1;
    out |= c << (2 * t);
  }
  return out;
}

// hash((x, y)) of CPython >= 3.8 for small non-negative ints (Objects/tupleobject.c: the
// xxHash-style tuplehash; hash(int) is the int) -- what orders list(set(locations)), see pyset_first
uint64_t py_hash_xy(int x, int y) {
  const uint64_t P1 = 11400714785074694791ULL, P2 = 14029467366897019727ULL, P5 = 2870177450012600261ULL;
  uint64_t acc = P5;
  const uint64_t lane[2] = {(uint64_t)x, (uint64_t)y};
  for (int k = 0; k < 2; k++) {
    acc += lane[k] * P2;
    acc = (acc << 31) | (acc >> 33);
    acc *= P1;
  }
  acc += 2ULL ^ (P5 ^ 3527539ULL);
  return acc == (uint64_t)-1 ? 1546275796ULL : acc;
}
// the first eight probe slots of a location in an 8-slot set table, 3 bits each
// (Objects/setobject.c set_add_entry: i = hash & 7, then i = (5 i + 1 + (perturb >>= 5)) & 7)
uint32_t probe_code(int x, int y) {
  const uint64_t h = py_hash_xy(x, y);
  uint64_t perturb = h;
  uint32_t i = (uint32_t)(h & 7), code = 0;
  for (int t = 0; t < 8; t++) {
    code |= i << (3 * t);
    perturb >>= 5;
    i = (uint32_t)((i * 5 + 1 + perturb) & 7);
  }
  return code;
}

// Level blob (include/oc_level.h) -> LevelHdr + RunCfg.  Host only, no device work.
// Returns NULL on success, else a message.
const char *build_header(const int32_t *b, int32_t n_words, LevelHdr &h, RunCfg &run,
                         int32_t *slot_out = nullptr, int32_t *goal_index_out = nullptr) {
  if (!b || n_words < OC_LV_HEADER_WORDS) return "null or short blob";
  if (b[OC_LV_MAGIC] != OC_LV_MAGIC_VALUE || b[OC_LV_VERSION] != OC_LV_VERSION_VALUE ||
      b[OC_LV_TOTAL] != n_words)
    return "bad magic/version/length";
  const int W = b[OC_LV_W], H = b[OC_LV_H], A = b[OC_LV_A], M = b[OC_LV_M], S = b[OC_LV_S];
  const int nc = W * H;
  if (W < 1 || H < 1 || W > 16 || H > 16 || nc > OC_MAX_CELLS || A < 2 || A > OC_MAX_AGENTS || M < 1 ||
      M > OC_MAX_ITEMS || S < 1 || S > OC_MAX_SUBTASKS || b[OC_LV_NPAIR] > OC_MAX_PAIR ||
      b[OC_LV_NDELIV] < 1 || b[OC_LV_NDELIV] > OC_MAX_DELIV || b[OC_LV_MAX_PATH] > 255 ||
      b[OC_LV_T] < 0 || b[OC_LV_T] > 0xFFFF)
    return "level dimensions out of range";
  memset(&h, 0, sizeof(h));
  h.W = W; h.H = H; h.A = A; h.M = M; h.S = S; h.max_path = b[OC_LV_MAX_PATH]; h.ncells = nc;
  run.T = b[OC_LV_T];
  run.inv_T = run.T ? 1.0 / (double)run.T : 0.0;
  run.inv_max_path = 1.0 / (double)b[OC_LV_MAX_PATH];
  run.allergic = (uint32_t)b[OC_LV_ALLERGIC];
  run.play = (uint32_t)(b[OC_LV_FLAGS] & OC_FLAG_PLAY);
  const int32_t *cells = b + b[OC_LV_OFF_CELLS];
  const int32_t *ag = b + b[OC_LV_OFF_AGENTS], *it = b + b[OC_LV_OFF_ITEMS];
  const int32_t *st = b + b[OC_LV_OFF_SUBTASKS], *pr = b + b[OC_LV_OFF_PAIR], *dl = b + b[OC_LV_OFF_DELIV];
  for (int c = 0; c < nc; c++) {
    const uint64_t bit = 1ull << (c & 63);
    if (cells[c] != OC_FLOOR) h.nonfloor[c >> 6] |= bit;
    if (cells[c] & 1) h.cell_lo[c >> 6] |= bit;
    if (cells[c] & 2) h.cell_hi[c >> 6] |= bit;
  }
  for (int f = 0; f < 3; f++) h.food_item[f] = 255;
  int type_count[OC_NTYPES] = {0, 0, 0, 0};
  for (int i = 0; i < M; i++) {
    const int t = it[3 * i];
    if (t < 0 || t >= OC_NTYPES) return "bad item type";
    if (i > 0 && t != it[3 * (i - 1)] && type_count[t] > 0) return "items must be grouped by type (world order)";
    type_count[t]++;
    if (t != OC_PLATE) {
      if (h.food_item[t] != 255) h.has_dup = 1;   // a food type occurs twice: dup mode
      else h.food_item[t] = (uint32_t)i;
      h.food_items[t] |= 1u << i;
    }
    h.item_types |= (uint32_t)t << (4 * i);
  }
  for (int t = 0; t < OC_NTYPES; t++)
    if (type_count[t] > 3) return "more than three items of one type";
  for (int s = 0; s < S; s++)
    for (int t = 0; t < OC_NTYPES; t++)
      if (((st[4 * s + 1] >> (4 * t)) & 15) > 1) h.has_dup = 1;   // a goal object repeats a content type
  if (h.has_dup) {
    // the names a merge can create: every multiset of >= 2 contents drawn from the level's
    // items with at most one Plate (mergeable(), utils/core.py:240-257, checks nothing else)
    const int cp = type_count[OC_PLATE] > 0 ? 1 : 0;
    for (int a = 0; a <= type_count[0]; a++)
      for (int b2 = 0; b2 <= type_count[1]; b2++)
        for (int c = 0; c <= type_count[2]; c++)
          for (int d = 0; d <= cp; d++)
            if (a + b2 + c + d >= 2) {
              if (h.nnames >= (uint32_t)MAX_NAMES) return "too many distinct merged object names";
              h.name_sig[h.nnames++] = (uint32_t)(a | (b2 << 2) | (c << 4) | (d << 6));
            }
  }
  // canonical subtask slots (see RunCfg): Chop / Merge subtasks sorted by (kind, goal object,
  // food), ties in the caller's order -- tied subtasks are indistinguishable to the kernels --
  // then the Deliver subtasks in the caller's order
  int order[OC_MAX_SUBTASKS], slot[OC_MAX_SUBTASKS], nord = 0;
  for (int pass = 0; pass < 2; pass++)
    for (int u = 0; u < S; u++)
      if ((st[4 * u] == OC_DELIVER) == (pass == 1)) order[nord++] = u;
  for (int i = 1; i < S; i++) {   // insertion sort of the non-Deliver prefix (stable)
    const int u = order[i];
    if (st[4 * u] == OC_DELIVER) break;
    int j = i;
    while (j > 0) {
      const int v = order[j - 1];
      const bool greater = st[4 * v] != st[4 * u] ? st[4 * v] > st[4 * u]
                           : st[4 * v + 1] != st[4 * u + 1] ? st[4 * v + 1] > st[4 * u + 1]
                                                            : st[4 * v + 2] > st[4 * u + 2];
      if (!greater) break;
      order[j] = v;
      j--;
    }
    order[j] = u;
  }
  run.slot_identity = 1;
  memset(run.slot4, 0, sizeof(run.slot4));
  for (int c = 0; c < S; c++) {
    slot[order[c]] = c;
    if (order[c] != c) run.slot_identity = 0;
  }
  for (int u = 0; u < S; u++) run.slot4[u >> 2] |= (uint32_t)slot[u] << (8 * (u & 3));
  for (int s = 0; s < S; s++) {   // s = canonical slot from here on
    const int u = order[s];
    const int kind = st[4 * u], sig = st[4 * u + 1], food = st[4 * u + 2];
    const int s7 = sig7_of_sig(sig);
    if (s7 < 0) return "goal object holds more than three of a food or two Plates";
    // goals are told apart by their multiset in dup mode, by their type set otherwise (the same
    // thing when nothing repeats)
    const int ts = h.has_dup ? s7 : tset_of_sig(sig);
    if (kind == OC_DELIVER) {
      h.deliver_mask |= 1u << s;
      if (h.ndel >= (uint32_t)MAX_DELS) return "too many Deliver subtasks";
      h.del_sig[h.ndel] = (uint32_t)s7;
      h.del_tset[h.ndel] = (uint32_t)ts;
      h.del_bit[h.ndel] = (uint32_t)s;
      h.ndel++;
    } else {
      h.nondeliver_mask |= 1u << s;
      if (kind == OC_CHOP) {
        if (food < 0 || food > 2 || h.food_item[food] == 255) return "Chop of an absent food";
        h.chop_mask[food] |= 1u << s;
      }
    }
    uint32_t g = 0;
    for (; g < h.ngoal; g++)
      if (h.goal_tset[g] == (uint32_t)ts) break;
    if (g == h.ngoal) {
      if (h.ngoal >= (uint32_t)MAX_GOALS) return "too many distinct goal objects";
      h.goal_sig[h.ngoal] = (uint32_t)s7;
      h.goal_tset[h.ngoal++] = (uint32_t)ts;
    }
    if (kind == OC_DELIVER) h.goal_dl[g] |= 1u << s; else h.goal_nd[g] |= 1u << s;
    if (slot_out) slot_out[u] = s;
    if (goal_index_out) goal_index_out[u] = (int32_t)g;
  }
  // pair term: Plate + recipe[0] ingredient names, every unordered pair in that order
  // (overcooked_environment.py:319-363); one distance lookup per item pair
  for (int p = 0; p < b[OC_LV_NPAIR]; p++)
    for (int q = p + 1; q < b[OC_LV_NPAIR]; q++) {
      int cnt = 0;
      for (int i = 0; i < M; i++)
        for (int j = 0; j < M; j++)
          if (it[3 * i] == pr[p] && it[3 * j] == pr[q]) {
            if (h.npairlk >= (uint32_t)MAX_PAIRLK) return "too many item pairs in the shaping pair term";
            h.pairlk[h.npairlk++] = (uint32_t)(i | (j << 4));
            cnt++;
          }
      if (cnt) h.pairlk[h.npairlk - 1] |= 1u << 8; else h.pair_static_max++;
    }
  h.ndeliv = (uint32_t)b[OC_LV_NDELIV];
  for (uint32_t k = 0; k < h.ndeliv; k++) h.deliv_pos[k] = (uint32_t)(dl[2 * k] | (dl[2 * k + 1] << 4));
  // initial state words: OvercookedEnvironment.reset() (overcooked_environment.py:180-206)
  for (int a = 0; a < A; a++) h.init_words[a] = ag[2 * a] | (ag[2 * a + 1] << 4);
  for (int i = 0; i < M; i++) {
    int first = i;   // first item of the same type: its key is created when that one is inserted
    while (first > 0 && it[3 * (first - 1)] == it[3 * i]) first--;
    const int seqf = h.has_dup ? ((first << 4) | i) : i;
    const int sigf = item_sig_bit(h.has_dup != 0, it[3 * i]);
    h.init_words[A + i] = it[3 * i + 1] | (it[3 * i + 2] << 4) | (i << 9) | (seqf << 16) | sigf;
  }
  {
    int n_chop = 0, n_groups = (int)h.pair_static_max;
    for (int f = 0; f < 3; f++) n_chop += __builtin_popcount(h.chop_mask[f]);
    for (uint32_t k = 0; k < h.npairlk; k++) n_groups += (h.pairlk[k] >> 8) & 1;
    int kmax = h.max_path + 64;                                          // Deliver term: distance + manhattan
    if (2 * n_chop * h.max_path > kmax) kmax = 2 * n_chop * h.max_path;  // Chop term numerator
    if (n_groups * h.max_path > kmax) kmax = n_groups * h.max_path;      // pair term numerator
    h.nquot = (uint32_t)(kmax + 2);
  }
  h.closed_border = border_closed(h) ? 1u : 0u;
  h.planes128 = nc > 64 ? 1u : 0u;
  h.nscatter = (uint32_t)b[OC_LV_NSCATTER];
  h.ncounters = (uint32_t)b[OC_LV_NCOUNTERS];
  if (h.nscatter > 4 || h.ncounters > OC_MAX_COUNTERS || (h.nscatter > 0 && h.ncounters < h.nscatter))
    return "bad scatter / Counter counts";
  for (uint32_t k = 0; k < h.nscatter; k++) {
    const int item = (b + b[OC_LV_OFF_SCATTER])[k];
    if (item < 0 || item >= M) return "bad scatter item index";
    h.scatter_item[k] = (uint32_t)item;
  }
  return nullptr;
}

// The STRUCTURE of a level (see OC_HDR_FIELDS): the header with the map's geometry blanked.  A
// specialised library is generated from, and checks new levels against, this part only.
LevelHdr structure_of(const LevelHdr &h) {
  LevelHdr t = h;
#define OC_KEEP(...)
#define OC_BLANK(T, name, ...) memset(&t.name, 0, sizeof(t.name));
  OC_HDR_FIELDS(OC_KEEP, OC_KEEP, OC_BLANK, OC_BLANK)
#undef OC_KEEP
#undef OC_BLANK
  return t;
}

// ---- the text of a specialised library's header ------------------------------------------------
struct Text {   // snprintf into a caller's buffer; n counts what the whole text needs
  char *buf;
  int size, n;
  __attribute__((format(printf, 2, 3))) void put(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    n += vsnprintf(buf + (n < size ? n : 0), n < size ? (size_t)(size - n) : 0, fmt, ap);
    va_end(ap);
  }
  void value(int32_t v) { put("%d", v); }
  void value(uint32_t v) { put("0x%xu", v); }
  void value(uint64_t v) { put("0x%llxull", (unsigned long long)v); }
  template <typename T, int N>
  void value(const T (&a)[N]) {
    put("{");
    for (int k = 0; k < N; k++) put(k ? ", " : ""), value(a[k]);
    put("}");
  }
};
// `constexpr LevelHdr OC_SPEC_HDR = {...};` -- one aggregate initialiser, a line per field of
// OC_HDR_FIELDS.  Returns the length of the text, which is complete only if that is < buf_size.
int spec_header_text(const LevelHdr &h, char *buf, int buf_size) {
  Text t{buf, buf_size, 0};
  t.put("// generated by oc_level_spec_source -- do not edit\nconstexpr LevelHdr OC_SPEC_HDR = {\n");
#define OC_EMIT(T, name, ...) t.put("  "), t.value(h.name), t.put(",  // " #name "\n");
  OC_HDR_FIELDS(OC_EMIT, OC_EMIT, OC_EMIT, OC_EMIT)
#undef OC_EMIT
  t.put("};\n");
  return t.n;
}

// ---- the host image of a level's device tables -------------------------------------------------
// [ncells * ncells] u8 path distances, padded to 16 bytes; then one u32 of set-table probe slots
// per cell (4 * OC_MAX_CELLS bytes: dup mode's set-order lookups); then, in the last
// OC_MAX_COUNTERS bytes, the Counter tiles (x | y<<4) for random placement.  (Until round-1 v11 a
// table of fp64 quotients k / max_path came first: oc_level.quot_bytes, now always 0.)
// `h` = build_header() of the same blob.  Returns NULL on success, else a message.
const char *build_tables(const int32_t *b, const LevelHdr &h, std::vector<uint8_t> &img) {
  const int nc = h.ncells;
  const int32_t *dist = b + b[OC_LV_OFF_DIST];
  const size_t bytes = (((size_t)nc * nc + 15) & ~(size_t)15) + 4 * OC_MAX_CELLS + OC_MAX_COUNTERS;
  img.assign(bytes, 0);
  for (int i = 0; i < nc * nc; i++) img[i] = (uint8_t)dist[i];
  uint8_t *probes = img.data() + bytes - OC_MAX_COUNTERS - 4 * OC_MAX_CELLS;
  for (int c = 0; c < nc; c++) {
    const uint32_t code = probe_code(c % h.W, c / h.W);
    memcpy(probes + 4 * c, &code, 4);
    // dup mode: eight stored probes must place a third location whatever two slots are taken
    uint32_t seen = 0;
    for (int t = 0; t < 8; t++) seen |= 1u << ((code >> (3 * t)) & 7);
    if (h.has_dup && __builtin_popcount(seen) < 3) return "a cell's set-table probe sequence is too short (dup mode)";
  }
  const int32_t *ct = b + b[OC_LV_OFF_COUNTERS];
  for (int k = 0; k < b[OC_LV_NCOUNTERS]; k++)
    img[bytes - OC_MAX_COUNTERS + k] = (uint8_t)(ct[2 * k] | (ct[2 * k + 1] << 4));
  return nullptr;
}
}  // namespace
