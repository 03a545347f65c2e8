// oc_step_device.h -- the device half of the stepper: per-env registers, predicates, reward
// shaping, env_step / env_obs, the kernel argument structs and every __global__ kernel.
// oc_kernels.hip includes it after oc_level_host.h (LevelHdr, RunCfg, OC_HDR_FIELDS) and launches
// what is defined here; the overview of the kernels' design heads that file.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/oc_hip.h"
#include "oc_level_host.h"
#include "oc_policy_device.h"

namespace {

#ifdef OC_STAMPS
// Diagnostic build only (never shipped, never timed): s_memtime stamps of the phases of
// k_multi_step, written by lane 0 of every wave to a debug buffer nothing else reads
// (cdna_hip_programming.md section 7, "In-kernel stamps").
#define OC_STAMP(k)                                                                  \
  do {                                                                               \
    unsigned long long t_;                                                           \
    __builtin_amdgcn_sched_barrier(0);                                               \
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");     \
    __builtin_amdgcn_sched_barrier(0);                                               \
    oc_tt[(k)] = t_;                                                                 \
  } while (0)
#define OC_STAMP_PARAM , unsigned long long (&oc_tt)[16]
#define OC_STAMP_PASS , oc_tt
#else
#define OC_STAMP(k) do { } while (0)
#define OC_STAMP_PARAM
#define OC_STAMP_PASS
#endif

#ifdef OC_TIMELINE
// Diagnostic build flavour (never the product, never the headline): every wave of k_step /
// k_multi_step reads the constant-rate 100 MHz counter (s_memrealtime: the same clock on every XCD,
// unlike the per-XCD shader clock of s_memtime) when it starts and when its last instruction has
// been issued, and lane 0 writes them -- and the wave's lifetime in shader-clock cycles -- to the
// wave's OWN 16 bytes of the launch's record, uint32 [stride][4].  A graph of chained launches
// replayed on such a build yields, per launch, the span in which the kernel had waves on the chip
// ("kernel-active") and the gap to the next launch's first wave (the launch boundary: store drain,
// end-of-kernel cache work, the command processor, the next dispatch) -- the split of ms_per_step
// that bench.py --decompose reports, without a profiler attached (include/oc_hip.h:
// oc_timeline_begin).  -DOC_TIMELINE=2 additionally waits for the wave's stores (s_waitcnt
// vmcnt(0)) and stamps that too: how much of the boundary is store drain.
// Earlier forms perturbed what they measured: same-address atomics (4 x 256 waves on one line:
// 14.6 us per launch instead of 3.1); a store wait + default-policy stamp stores in every wave
// (+0.45 us: the wave outlives its stores and leaves dirty lines for the end-of-kernel write-back);
// four 8-byte write-through stores per wave (+0.2 us at 4 096 envs, +1 us at 131 072).  Now: ONE
// 16-byte write-through store per wave.
#define OC_TL_BEGIN()                                                            \
  const unsigned long long oc_tl0_ = __builtin_amdgcn_s_memrealtime();           \
  const unsigned long long oc_tc0_ = __builtin_amdgcn_s_memtime()
#define OC_TL_END(ptr_, stride_, ln_)                                                            \
  do {                                                                                           \
    __builtin_amdgcn_sched_barrier(0);                                                           \
    const unsigned long long oc_tl1_ = __builtin_amdgcn_s_memrealtime();                         \
    unsigned long long oc_tl2_ = oc_tl1_;                                                        \
    if (OC_TIMELINE >= 2) {                                                                      \
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                           \
      oc_tl2_ = __builtin_amdgcn_s_memrealtime();                                                \
    }                                                                                            \
    const unsigned long long oc_tc2_ = __builtin_amdgcn_s_memtime();                             \
    unsigned long long *tl_ = (ptr_);                                                            \
    /* (a lane-split launch, ln_ workgroups per 64 envs: every ln_-th workgroup writes, so the   \
       record keeps its 4 * ceil(n / 64) waves -- a SAMPLE of the launch's waves) */             \
    if (tl_ != nullptr && (threadIdx.x & 63) == 0 && blockIdx.x % (ln_) == 0) {                  \
      /* ONE 16-byte write-through store per wave: {start (64 bits), issue-end - start | (drain-end  \
         - start) << 16, shader cycles}; spans are < 65 536 ticks (655 us) */                     \
      typedef int v4i_ __attribute__((ext_vector_type(4)));                                      \
      const int64_t w_ = (int64_t)(blockIdx.x / (ln_)) * (blockDim.x >> 6) + (threadIdx.x >> 6); \
      const __amdgpu_buffer_rsrc_t r_ = __builtin_amdgcn_make_buffer_rsrc(tl_, 0, 0x7FFFFFFF, 0x00020000); \
      const unsigned d1_ = (unsigned)min((unsigned long long)0xFFFF, oc_tl1_ - oc_tl0_);         \
      const unsigned d2_ = (unsigned)min((unsigned long long)0xFFFF, oc_tl2_ - oc_tl0_);         \
      v4i_ q_;                                                                                   \
      q_.x = (int)(unsigned)oc_tl0_;                                                             \
      q_.y = (int)(unsigned)(oc_tl0_ >> 32);                                                     \
      q_.z = (int)(d1_ | (d2_ << 16));                                                           \
      q_.w = (int)(unsigned)(oc_tc2_ - oc_tc0_);                                                 \
      __builtin_amdgcn_raw_buffer_store_b128(q_, r_, (int)w_ * 16, 0, 16);                       \
    }                                                                                            \
  } while (0)
#else
#define OC_TL_BEGIN() do { } while (0)
#define OC_TL_END(ptr_, stride_, ln_) do { } while (0)
#endif

// The kernels read the level through ACCESSORS (L.W(), L.goal_tset(g), ...), generated from the
// one list of fields (OC_HDR_FIELDS, oc_level_host.h) for two header classes.  The fields come in
// two kinds:
//   STRUCTURE  what the recipes and the item multiset fix -- subtask masks, goal objects, item
//              types, the shaping lookup programs, the two map flags above;
//   GEOMETRY   the map itself -- size, tile bit-planes, Delivery positions, start cells (the
//              distance and Counter tables are device buffers anyway).
//   HdrC  specialised build: STRUCTURE accessors return fields of the constexpr OC_SPEC_HDR, so
//         loop bounds, type tests and masks fold at compile time.  GEOMETRY accessors come in
//         two flavours of library:
//           -DOC_SPEC_GEOMETRY  ("level" library) constexpr as well: everything folds, the
//               fastest code (3.64 us per step, tomato-2 x 4096), valid for ONE map;
//           otherwise           ("structure" library) they read the by-value kernel argument (a
//               dozen scalar loads; 3.82 us): the library is keyed by the STRUCTURE alone, so
//               every map with the same recipes, item multiset, agent count and border kind
//               runs on it -- all `*_tomato` levels share one, and so does a user-made map with
//               those recipes on a box that has no hipcc (the generic library takes 7.3 us).
//   HdrK  generic build: both kinds are scalar loads from the kernel arguments.
// (Tried and dropped in round 2: the header spread over the lanes of three VGPRs, one
// v_readlane per access.  Slower -- 7.68 us per step at 4 096 envs against 6.97 us with kernarg
// loads: ~290 readlanes with their SGPR-hazard wait states cost more than the scalar-cache hits
// they replace -- and unsafe: the compiler may copy such a VGPR under a partial EXEC mask, which
// loses the words parked in inactive lanes.)
#define OC_KF(T, name) __device__ __forceinline__ T name() const { return k.name; }
#define OC_KA(T, name, N) __device__ __forceinline__ T name(int i) const { return k.name[i]; }
#ifdef OC_SPECIALIZED
#include OC_SPEC_FILE  // constexpr LevelHdr OC_SPEC_HDR = {...};
struct HdrC {
  const LevelHdr &k;   // the by-value kernel argument: the map's geometry
#define OC_F(T, name) __device__ __forceinline__ constexpr T name() const { return OC_SPEC_HDR.name; }
#define OC_A(T, name, N) __device__ __forceinline__ constexpr T name(int i) const { return OC_SPEC_HDR.name[i]; }
#ifdef OC_SPEC_GEOMETRY
  OC_HDR_FIELDS(OC_F, OC_A, OC_F, OC_A)
#else
  OC_HDR_FIELDS(OC_F, OC_A, OC_KF, OC_KA)
#endif
#undef OC_F
#undef OC_A
};
using Hdr = HdrC;
#define OC_HDR_LOAD(args) const HdrC L {(args).L}
#else
struct HdrK {
  const LevelHdr &k;   // the by-value kernel argument
  OC_HDR_FIELDS(OC_KF, OC_KA, OC_KF, OC_KA)
};
using Hdr = HdrK;
#define OC_HDR_LOAD(args) const HdrK L {(args).L}
#endif
#undef OC_KF
#undef OC_KA

// ---------------------------------------------------------------------------
// per-env registers
// ---------------------------------------------------------------------------
// Items stay PACKED in registers exactly as they sit in the state tensor (include/oc_hip.h):
//   x | y<<4 | chopped<<8 | group<<9 | (holder+1)<<12 | seq<<16 | tset<<24
// Every item of one Object carries the same group / seq / tset, and on a non-Delivery cell at
// most one unheld Object exists, so "the held Object" and "the Object on the target cell" are
// plain ORs over the matching item words, a field test is one AND + compare on the word, and
// an update of several fields is one bit-field insert (v_bfi_b32).
constexpr int IW_POS = 0x000000FF, IW_CHOP = 0x00000100, IW_GRP = 0x00000E00, IW_HOLD = 0x00007000,
              IW_SEQ = 0x00FF0000, IW_TSET = 0x0F000000;
// "dup" mode (template bool DUP; a level that repeats a content type): bits 24..30 hold the
// Object's content COUNTS instead of its type set -- T | L<<2 | O<<4 (two bits each, at most
// three of a food) | P<<6 -- and bits 16..23 hold kseq<<4 | seq: seq = the Object's insertion
// number as before (4 bits are enough: at most M - 1 <= 7 merges per episode), kseq = the seq of
// the FIRST Object ever inserted under the same name this episode, i.e. the creation rank of its
// key in the reference's dict of lists (utils/world.py:21,236-237).  world.objects iterates key
// by key, so the composite is the world-order rank -- and equals seq<<4 | seq whenever every
// name is created at most once, which is why non-dup levels never needed it.
template <bool DUP>
constexpr int TS = DUP ? 0x7F000000 : IW_TSET;
template <bool DUP>
constexpr int OBJ = IW_GRP | IW_SEQ | TS<DUP>;   // what a merge rewrites
template <bool DUP>
__host__ __device__ constexpr int sig_of_type(int t) { return DUP ? (1 << (24 + 2 * t)) : (1 << (24 + t)); }

template <int A, int M, bool DUP>
struct Env {
  int ap[A], ahp[A];   // agent cell (x | y<<4); held group + 1 (0 = empty hands)
  int iw[M];           // packed item words
  int t, completed, goalcnt, mctr, err;
  int kn[2];           // DUP: 4 bits per merged name = 1 + seq of the first Object created under it (0 = never)
};
template <int A, int M, bool DUP>
constexpr int state_words() { return A + M + 2 + (DUP ? 2 : 0); }

__device__ __forceinline__ int ipos(int w) { return w & IW_POS; }
__device__ __forceinline__ int ichop(int w) { return (w >> 8) & 1; }
__device__ __forceinline__ int igrp(int w) { return (w >> 9) & 7; }
__device__ __forceinline__ int iseq(int w) { return (w >> 16) & 255; }
__device__ __forceinline__ int itset(int w) { return (w >> 24) & 15; }
__device__ __forceinline__ int bfi(int mask, int a, int b) { return (a & mask) | (b & ~mask); }  // v_bfi_b32

template <int A, int M, bool DUP>
__device__ __forceinline__ void unpack(Env<A, M, DUP> &e, const int32_t *w) {
#pragma unroll
  for (int a = 0; a < A; a++) {
    e.ap[a] = w[a] & 255;
    e.ahp[a] = (w[a] >> 8) & 15;
  }
#pragma unroll
  for (int i = 0; i < M; i++) e.iw[i] = w[A + i];
  e.t = (w[0] >> 16) & 0xFFFF;
  e.mctr = (w[1] >> 16) & 255;
  e.err = (w[1] >> 24) & 255;
  e.completed = w[A + M];
  e.goalcnt = w[A + M + 1];
  if constexpr (DUP) e.kn[0] = w[A + M + 2], e.kn[1] = w[A + M + 3];
}

template <int A, int M, bool DUP>
__device__ __forceinline__ void pack(const Env<A, M, DUP> &e, int32_t *w) {
#pragma unroll
  for (int a = 0; a < A; a++) w[a] = e.ap[a] | (e.ahp[a] << 8);
  w[0] |= e.t << 16;
  w[1] |= (e.mctr << 16) | (e.err << 24);
#pragma unroll
  for (int i = 0; i < M; i++) w[A + i] = e.iw[i];
  w[A + M] = e.completed;
  w[A + M + 1] = e.goalcnt;
  if constexpr (DUP) w[A + M + 2] = e.kn[0], w[A + M + 3] = e.kn[1];
}

// ---------------------------------------------------------------------------
// per-lane predicates as VALU words
// ---------------------------------------------------------------------------
// A per-lane `bool` of the compiler lives in an SGPR pair (v_cmp -> s[n:n+1]) and its logic runs on
// the scalar unit (s_and_b64 / s_or_b64 ...), to come back through v_cndmask.  On gfx950 a scalar
// instruction that reads an SGPR a VECTOR instruction has just written stalls a lone wave ~16
// cycles (tools/issue_probe.hip, one wave on a SIMD: v_cmp + s_and = 24 cycles, the chain v_cmp ->
// s_and -> v_cndmask 28; the same decision on 0 / -1 words in VGPRs -- v_cmp/v_cndmask or
// v_bfe_i32 to make the word, v_and / v_or / v_bitop3 for the logic, v_bfi to select -- 4 per
// instruction), and interact()'s decision tree is a few hundred such hops: the step kernels ran
// at ~7 cycles per instruction where 4 is the issue rate.  So every per-lane predicate of the hot
// path is a P: an int that is 0 or -1, made opaque to the optimiser where it is born (`hide`:
// an empty asm; otherwise InstCombine folds and/or of sign-extended compares back into i1 logic
// and the backend selects the scalar unit again).
typedef int P;
// s_waitcnt vmcnt(0) as the operand of __builtin_amdgcn_s_waitcnt (gfx9 encoding: vmcnt in bits 3:0 and
// 15:14, expcnt 6:4 and lgkmcnt 11:8 left at their maxima): a wait the compiler's wait-count pass sees
constexpr int WAIT_VMCNT0 = 0x0F70;
__device__ __forceinline__ int hide(int v) {
  asm("" : "+v"(v));
  return v;
}
// How a P is born.  v_cmp + v_cndmask(0, -1) is two instructions, but every v_cmp writes vcc -- one
// register for all of them, so the pairs cannot interleave -- and a v_cndmask reading it needs two
// wait states behind the compare (the 3-agent kernel carried 80 s_nop).  For operands in
// [0, 2^31) -- every field of the packed state -- the sign of a difference is the predicate:
// two plain, independent VALU instructions (v_xad_u32 / v_sub + v_ashrrev_i32), no vcc, no nop.
// (The difference is hidden as well, in front of the shift: where the optimiser knows the operand's
// range -- a masked field, a bit-field extract -- it proves the sign test equal to a compare with
// zero and selects v_cmp + v_cndmask again, or a carry-out into vcc.)
__device__ __forceinline__ P sign_of(int d) { return hide(hide(d) >> 31); }
__device__ __forceinline__ P p_z(int a) { return sign_of((int)((unsigned)a - 1u)); }              // a == 0   (a >= 0)
__device__ __forceinline__ P p_nz(int a) { return sign_of((int)(0u - (unsigned)a)); }             // a != 0   (a >= 0)
__device__ __forceinline__ P p_eq(int a, int b) { return sign_of((int)((unsigned)(a ^ b) - 1u)); }  // (bit 31 of a, b equal)
__device__ __forceinline__ P p_ne(int a, int b) { return ~p_eq(a, b); }
__device__ __forceinline__ P p_lt(int a, int b) { return sign_of(a - b); }                        // a < b    (0 <= a, b < 2^31)
__device__ __forceinline__ P p_gt(int a, int b) { return p_lt(b, a); }
__device__ __forceinline__ P p_ge(int a, int b) { return ~p_lt(a, b); }
__device__ __forceinline__ P p_le(int a, int b) { return ~p_lt(b, a); }
// ... and for operands of any value (caller-supplied action indices, 32-bit subtask masks): the compare
__device__ __forceinline__ P p_eq_any(int a, int b) { return hide(a == b ? -1 : 0); }
__device__ __forceinline__ P p_gtu_any(unsigned a, unsigned b) { return hide(a > b ? -1 : 0); }
__device__ __forceinline__ P p_geu_any(unsigned a, unsigned b) { return hide(a >= b ? -1 : 0); }
__device__ __forceinline__ P p_ltu_any(unsigned a, unsigned b) { return hide(a < b ? -1 : 0); }
// bit k as 0 / -1: one v_bfe_i32 (hidden: a visible extract is re-derived where it is consumed, as
// shift + compare + select in a `sel`, as and + compare under a `~`)
__device__ __forceinline__ P p_bit(int w, unsigned k) { return hide(__builtin_amdgcn_sbfe(w, k, 1u)); }
__device__ __forceinline__ P p_of(bool uniform) { return uniform ? -1 : 0; }                       // a wave-uniform condition
__device__ __forceinline__ int sel(P m, int a, int b) { return (a & m) | (b & ~m); }               // v_bfi_b32

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
// |a - b| + c on unsigned operands in one instruction (hipcc expands __sad() into compare,
// two subtracts, select and add)
__device__ __forceinline__ unsigned sad_u32(unsigned a, unsigned b, unsigned c) {
  unsigned r;
  asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ int manhattan(int p, int q) {   // packed cells x | y<<4
  return (int)sad_u32((unsigned)(p & 15), (unsigned)(q & 15), sad_u32((unsigned)(p >> 4), (unsigned)(q >> 4), 0u));
}
__device__ __forceinline__ int px(int p) { return p & 15; }
__device__ __forceinline__ int py(int p) { return p >> 4; }
__device__ __forceinline__ int dense(const Hdr &L, int p) {
  // y * W + x from p = x + 16 y without unpacking x: p - (16 - W) * y  (v_lshrrev + v_mad_i32_i24)
  return __mul24(py(p), L.W() - 16) + p;
}
// bit c of a 128-bit plane held as two 64-bit words
__device__ __forceinline__ int bit128(uint64_t w0, uint64_t w1, int c) {
  const uint64_t v = (c & 64) ? w1 : w0;
  return (int)((v >> (c & 63)) & 1);
}
__device__ __forceinline__ int item_type(const Hdr &L, int i) { return (L.item_types() >> (4 * i)) & 15; }
// tile type (OC_FLOOR / COUNTER / CUTBOARD / DELIVERY) of dense cell c
__device__ __forceinline__ int cell_type(const Hdr &L, int c) {
  if (!L.planes128())  // uniform (compile-time in specialised builds): one 64-bit plane each
    return (int)((L.cell_lo(0) >> c) & 1) | ((int)((L.cell_hi(0) >> c) & 1) << 1);
  return bit128(L.cell_lo(0), L.cell_lo(1), c) | (bit128(L.cell_hi(0), L.cell_hi(1), c) << 1);
}

#ifdef OC_SPECIALIZED
constexpr bool OC_BORDER_CLOSED = OC_SPEC_HDR.closed_border != 0;   // (set by build_header from the map)
#else
constexpr bool OC_BORDER_CLOSED = false;
#endif

// t / T as CPython computes it (overcooked_env.py:146: int / int, correctly rounded fp64)
// without the 11-instruction fp64 division: q0 = t * RN(1/T), one FMA for the exact
// residual, one FMA to correct.  Equal to the division for every 0 <= t, 1 <= T <= 65535
// (all 4.3e9 pairs compared bit for bit: tests/test_host_cpu.py, tools/div_check.c).
// No time limit (T == 0, uniform): t / 0.0, i.e. nan for t == 0 and inf otherwise, selected over the
// quotient word by word under a uniform mask -- straight-line code, so that a caller can form the
// value among its other arithmetic (as an early return it was three branches, and the kernels
// carried the whole function behind their last row store).
__device__ __forceinline__ double timestep_of(int t, const RunCfg &R) {
  typedef int v2i __attribute__((ext_vector_type(2)));
  const double dt = (double)t;
  const double q0 = dt * R.inv_T;
  const double r = __builtin_fma(-(double)R.T, q0, dt);
  const v2i q = __builtin_bit_cast(v2i, __builtin_fma(r, R.inv_T, q0));
  const P unlimited = p_of(R.T == 0);
  const int hi0 = 0x7FF00000 | (p_z(t) & 0x00080000);   // inf; nan: the bits of __builtin_nan("")
  v2i out;
  out.x = q.x & ~unlimited;
  out.y = sel(unlimited, hi0, q.y);
  return __builtin_bit_cast(double, out);
}


// An [R][n] tensor of 4-byte (or 8-byte) elements addressed through a buffer resource:
// the per-lane part of the address is one 32-bit byte offset (voffset), the row offset is
// a scalar (soffset), so a row access costs no vector address arithmetic at all.  The
// descriptor's record count bounds the whole tensor; the tail lanes of the last wave are
// still masked by the caller because rows are contiguous.
//
// AUX = cache-policy bits of the stores (bit 0 sc0, bit 1 nt, bit 4 sc1).  With sc1 (agent
// scope) the L2 writes a line through to the fabric at once instead of holding it dirty
// until the end-of-kernel write-back, so the write-back overlaps the rest of the launch
// instead of trailing it.  tools/store_probe.hip (76 row stores per env): 10.4 -> 7.9 us
// per launch at n = 131072, 4.4 -> 3.7 us at 32768; sc0 / nt change nothing.  In the
// kernels (round 1, v5): salad-2 x 32768 6.84 -> 5.88 us, tomato-2 x 131072 11.1 -> 10.0 us, but
// 4.56 -> 4.66 us at n = 4096 -- back then every wave still ended on a wait for its own stores
// (the metrics slot was a load + store), and a lone wave per CU waited longer for a written-
// through one.  Since v11 no wave waits for its stores, and round 2 re-measured
// (tools/wt_threshold.sh): write-through is never slower, 3.64 -> 3.51 us at n = 4096, 3.53 ->
// 3.46 us at 512, 3.44 -> 3.43 us at 64, salad-2 x 4096 3.89 -> 3.74 us.  The launcher picks the
// write-through variant (template bool WT) at every batch size; OC_LAUNCH=wt=0 restores
// write-back stores.
template <int AUX>
struct RowsT {
  __amdgpu_buffer_rsrc_t rsrc;
  int voff;      // lane byte offset inside a row
  int rowbytes;  // n * element size
  __device__ __forceinline__ RowsT(const void *base, int64_t n, int rows, int64_t i, int elem = 4) {
    rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, (int)(n * rows * elem), 0x00020000);
    voff = (int)i * elem;
    rowbytes = (int)n * elem;
  }
  __device__ __forceinline__ int ld(int row) const {
    return __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, row * rowbytes, 0);
  }
  __device__ __forceinline__ void st(int row, int v) const {
    __builtin_amdgcn_raw_buffer_store_b32(v, rsrc, voff, row * rowbytes, AUX);
  }
  __device__ __forceinline__ void st8(int row, int v) const {   // rows of 1-byte elements
    __builtin_amdgcn_raw_buffer_store_b8((char)v, rsrc, voff, row * rowbytes, AUX);
  }
  __device__ __forceinline__ void st_f64(int row, double v) const {
    typedef int v2i __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2i, v), rsrc, voff, row * rowbytes, AUX);
  }
  // a run of rows stored from a loop: the caller carries the row's byte offset along (soff(first
  // row), += rowbytes per row) instead of multiplying for every row
  __device__ __forceinline__ int soff(int row) const { return row * rowbytes; }
  __device__ __forceinline__ void st_at(int so, int, int v) const {
    __builtin_amdgcn_raw_buffer_store_b32(v, rsrc, voff, so, AUX);
  }
  __device__ __forceinline__ void st8_at(int so, int, int v) const {
    __builtin_amdgcn_raw_buffer_store_b8((char)v, rsrc, voff, so, AUX);
  }
};
// One viewer's rows of the observation tensor with the byte offsets of its first N rows held in
// SGPRs: so[k] = (row0 + k) * rowbytes.  The caller forms them (a chain of adds) where it has
// nothing else to do -- a split workgroup's observation waves, under the wait for the state in
// front of the barrier -- so that the ~30 row stores at the end of the step are not each
// preceded by a scalar multiply: a lone wave pays ~4 cycles for every instruction it issues,
// whatever its type (tools/issue_probe.hip).  Rows are named as everywhere else, by their index
// in the tensor; every store of one of the first N rows must name it by a compile-time offset
// from row0 (straight-line or fully unrolled code), or the table would have to live in memory.
template <int AUX, int N>
struct RowsPreT : RowsT<AUX> {   // (N == 0: no table, a plain RowsT)
  int so[N > 0 ? N : 1];
  int row0;
  __device__ __forceinline__ RowsPreT(const RowsT<AUX> &rows, int row0_) : RowsT<AUX>(rows), row0(row0_) {
    [[maybe_unused]] int o = row0_ * rows.rowbytes;
#pragma unroll
    for (int k = 0; k < N; k++) {
      so[k] = o;
      asm volatile("" : "+s"(so[k]));   // formed HERE, held until its store
      o = so[k] + rows.rowbytes;
    }
  }
  __device__ __forceinline__ int off(int row) const {
    const int k = row - row0;
    return (k >= 0 && k < N) ? so[k] : row * this->rowbytes;
  }
  __device__ __forceinline__ void st(int row, int v) const {
    __builtin_amdgcn_raw_buffer_store_b32(v, this->rsrc, this->voff, off(row), AUX);
  }
  __device__ __forceinline__ void st8(int row, int v) const {
    __builtin_amdgcn_raw_buffer_store_b8((char)v, this->rsrc, this->voff, off(row), AUX);
  }
  // the same with the lane's byte offset given by the caller: a lane-split launch (LaneParts) adds
  // the distance to its part's row to it, so ONE store writes a different row in every part
  __device__ __forceinline__ void st_v(int row, int vo, int v) const {
    __builtin_amdgcn_raw_buffer_store_b32(v, this->rsrc, vo, off(row), AUX);
  }
  __device__ __forceinline__ void st8_v(int row, int vo, int v) const {
    __builtin_amdgcn_raw_buffer_store_b8((char)v, this->rsrc, vo, off(row), AUX);
  }
};
// RowsT that also leaves every stored value, as a float, in an LDS image [row - rowbase][64 lanes]:
// how a split workgroup's observation waves hand a viewer's rows to the waves that evaluate the
// policies (multi_step_body, POL) without a trip through memory.  OT: 0 int32, 1 int8, 2 float32 bits.
template <int AUX, int OT>
struct RowsLdsT : RowsT<AUX> {
  float *lds;
  int rowbase, lane;
  __device__ __forceinline__ RowsLdsT(const RowsT<AUX> &rows, float *lds_, int rowbase_, int lane_)
      : RowsT<AUX>(rows), lds(lds_), rowbase(rowbase_), lane(lane_) {}
  __device__ __forceinline__ void st(int row, int v) const {
    RowsT<AUX>::st(row, v);
    lds[(row - rowbase) * 64 + lane] = OT == 2 ? __builtin_bit_cast(float, v) : (float)v;
  }
  __device__ __forceinline__ void st8(int row, int v) const {
    RowsT<AUX>::st8(row, v);
    lds[(row - rowbase) * 64 + lane] = (float)v;
  }
  __device__ __forceinline__ void st_at(int so, int row, int v) const {
    RowsT<AUX>::st_at(so, row, v);
    lds[(row - rowbase) * 64 + lane] = OT == 2 ? __builtin_bit_cast(float, v) : (float)v;
  }
  __device__ __forceinline__ void st8_at(int so, int row, int v) const {
    RowsT<AUX>::st8_at(so, row, v);
    lds[(row - rowbase) * 64 + lane] = (float)v;
  }
};
using Rows = RowsT<0>;          // loads and default-policy stores
#ifndef OC_AUX_WT
#define OC_AUX_WT 16            // sc1; -DOC_AUX_WT=<bits> via OC_HIP_EXTRA_FLAGS to try other store policies
#endif
constexpr int AUX_WT = OC_AUX_WT;

// calculate_reward_shaping for sim agents 0 and 1 (overcooked_environment.py:272-397),
// given the agents' cells, the item cells, the completed flags and, per Deliver subtask, the
// cell of its (all-chopped) object if one exists.  The int/int divisions of the reference
// are entries of the quotient table k / MAX_PATH; sums run left to right in fp64.
//
// Split so the kernels can order their memory operations: shaping_issue_pos/_del() form the
// addresses and issue the path-distance loads; shaping_lookup() consumes the distances and
// issues the quotient loads -- still ahead of the observation stores, because vmcnt retires
// loads and stores in issue order; shaping_sum() does the fp64 adds after the stores.
template <int B>
struct ShapeIn {   // what shaping_lookup() / shaping_sum() still need of the pre-reset env
  int ap[B];
  int completed;
  int del_has[MAX_DELS], del_p[MAX_DELS];
  int chop_p[3];   // DUP: the cell of "the" fresh food of each type (the set's element [0])
};

// ---------------------------------------------------------------------------
// dup mode: which location does list(set(locations))[0] return?
// ---------------------------------------------------------------------------
// World.get_all_object_locs is list(set(held_locs + unheld_locs)) (utils/world.py:290-291) and
// calculate_reward_shaping walks to element [0] of it (overcooked_environment.py:287,374-379).
// With several matching objects that is the location in the LOWEST SLOT of CPython's 8-slot set
// table: slot = hash((x, y)) & 7, a taken slot sends the newcomer along its probe sequence
// i <- (5 i + 1 + (perturb >>= 5)) & 7 (Objects/setobject.c; no linear probing in an 8-slot
// table; the table only grows at the fifth element and at most three objects can match).  The
// host stores each cell's first eight probe slots, 3 bits each, in a u32 table (`probe`) and
// checks at level creation that eight are enough for every triple of cells.
// cand[i]: item i is the representative of a matching Object.  Insertion order: held Objects
// first, then unheld ones, each in the order of the name's list = ascending seq field.
template <int M>
__device__ __forceinline__ int pyset_first(const Hdr &L, const uint32_t *__restrict__ probe,
                                           const int (&iw)[M], const bool (&cand)[M], int &has) {
  constexpr int BIG = 1 << 20;
  int ord[M];
#pragma unroll
  for (int i = 0; i < M; i++)
    ord[i] = cand[i] ? (((iw[i] & IW_HOLD) ? 0 : 256) | ((iw[i] >> 16) & 255)) : BIG;
  int cell[3], code[3];
  bool valid[3];
  int prev = -1;
#pragma unroll
  for (int k = 0; k < 3; k++) {   // the k-th candidate in insertion order
    int cur = BIG, c = 0;
#pragma unroll
    for (int i = 0; i < M; i++) {
      const bool better = ord[i] > prev && ord[i] < cur;
      cur = better ? ord[i] : cur;
      c = better ? ipos(iw[i]) : c;
    }
    valid[k] = cur != BIG;
    cell[k] = c;
    prev = valid[k] ? cur : BIG;
  }
  has = valid[0];
  if (__ballot(valid[1]) == 0) return cell[0];   // one match in every env of the wave: no set order to ask for
  // a location already in the set is not inserted again
  valid[1] = valid[1] && cell[1] != cell[0];
  valid[2] = valid[2] && cell[2] != cell[0] && !(valid[1] && cell[2] == cell[1]);
#pragma unroll
  for (int k = 0; k < 3; k++) code[k] = valid[k] ? (int)probe[dense(L, cell[k])] : 0;
  const int s0 = code[0] & 7;
  int s1 = 8, s2 = 8;
  // first free slot along each newcomer's probe sequence (scanned backwards, so the earliest
  // probe that is free is the one that stays)
#pragma unroll
  for (int t = 7; t >= 0; t--) {
    const int q1 = (code[1] >> (3 * t)) & 7;
    s1 = (q1 != s0) ? q1 : s1;
  }
  s1 = valid[1] ? s1 : 8;
#pragma unroll
  for (int t = 7; t >= 0; t--) {
    const int q2 = (code[2] >> (3 * t)) & 7;
    s2 = (q2 != s0 && q2 != s1) ? q2 : s2;
  }
  s2 = valid[2] ? s2 : 8;
  int best = cell[0], bs = s0;
  best = s1 < bs ? cell[1] : best;
  bs = min(bs, s1);
  best = s2 < bs ? cell[2] : best;
  return best;
}
template <int B>
struct ShapeLoads {   // raw path distances, in flight until shaping_lookup()
  int d_chop[3][B];
  int d_pair[MAX_PAIRLK];
  int d_del[MAX_DELS][B];
  int d_tile[OC_MAX_DELIV][B];
};

// The lookups that only need positions (Chop, pair and Delivery-tile terms): issued right after
// interact(), a hundred instructions before the rest, so they are back when shaping_lookup()
// wants them.  Table offsets are unsigned 24-bit products: full-rate v_mul_u32_u24 /
// v_mad_u32_u24 and a 32-bit offset on a scalar base (no 64-bit address arithmetic per lookup).
template <int B, int M, bool DUP>
__device__ __forceinline__ void shaping_issue_pos(const Hdr &L, const uint8_t *__restrict__ dist,
                                                  const ShapeIn<B> &in, const int (&ipos)[M], ShapeLoads<B> &ld) {
  const unsigned nc = (unsigned)L.ncells();
  unsigned arow[B];
#pragma unroll
  for (int b = 0; b < B; b++) arow[b] = __umul24((unsigned)dense(L, in.ap[b]), nc);
  unsigned ic[M];
#pragma unroll
  for (int i = 0; i < M; i++) ic[i] = (unsigned)dense(L, ipos[i]);
#pragma unroll
  for (int f = 0; f < 3; f++) {
#pragma unroll
    for (int b = 0; b < B; b++) ld.d_chop[f][b] = 0;
    if (L.chop_mask(f) != 0) {  // uniform
      unsigned fc = 0;
      if constexpr (DUP) {
        fc = (unsigned)dense(L, in.chop_p[f]);
      } else {
#pragma unroll
        for (int i = 0; i < M; i++) fc = ((int)L.food_item(f) == i) ? ic[i] : fc;
      }
#pragma unroll
      for (int b = 0; b < B; b++) ld.d_chop[f][b] = dist[arow[b] + fc];
    }
  }
#pragma unroll
  for (int k = 0; k < MAX_PAIRLK; k++) {
    ld.d_pair[k] = 0;
    if (k < (int)L.npairlk()) {  // uniform
      const int li = L.pairlk(k) & 15, lj = (L.pairlk(k) >> 4) & 15;
      unsigned ci = 0, cj = 0;
#pragma unroll
      for (int i = 0; i < M; i++) {
        ci = (li == i) ? ic[i] : ci;
        cj = (lj == i) ? ic[i] : cj;
      }
      ld.d_pair[k] = dist[__umul24(ci, nc) + cj];
    }
  }
#pragma unroll
  for (int k = 0; k < OC_MAX_DELIV; k++) {
#pragma unroll
    for (int b = 0; b < B; b++) ld.d_tile[k][b] = 0;
    if (k < (int)L.ndeliv()) {  // uniform
      const unsigned dc = (unsigned)dense(L, (int)L.deliv_pos(k));
#pragma unroll
      for (int b = 0; b < B; b++) ld.d_tile[k][b] = dist[arow[b] + dc];
    }
  }
}

// The Deliver-term lookups need the cell of each Deliver subtask's object (known after
// done/reward).
template <int B>
__device__ __forceinline__ void shaping_issue_del(const Hdr &L, const uint8_t *__restrict__ dist,
                                                  const ShapeIn<B> &in, ShapeLoads<B> &ld) {
  const unsigned nc = (unsigned)L.ncells();
#pragma unroll
  for (int k = 0; k < MAX_DELS; k++) {
#pragma unroll
    for (int b = 0; b < B; b++) ld.d_del[k][b] = 0;
    if (k < (int)L.ndel()) {  // uniform
      const unsigned mc = (unsigned)dense(L, in.del_p[k]);
#pragma unroll
      for (int b = 0; b < B; b++) ld.d_del[k][b] = dist[__umul24((unsigned)dense(L, in.ap[b]), nc) + mc];
    }
  }
}

// quotient values between shaping_lookup() and shaping_sum()
template <int B>
struct ShapeQ {
  double q_chop[B], q_pair, q_del[MAX_DELS][B];
  int nchop, npairs;
  bool del_direct[MAX_DELS][B];
};

// second part: consume the path distances (integer min / select logic) and form the
// quotients.  (Until round-1 v11 the quotients were table lookups, issued here -- ahead of the
// observation stores, because vmcnt retires loads and stores in issue order.)
// k / MAX_PATH as CPython computes it (int / int, correctly rounded fp64) by the two-FMA
// construction of timestep_of(): exact for every 0 <= k <= 65535, 1 <= MAX_PATH <= 65535
// (tools/div_check.c).  Replaces a table lookup -- five to seven global loads per env-step
// that had to be ordered around the stores.
__device__ __forceinline__ double quotient(int k, const Hdr &L, double inv_max_path) {
  const double dk = (double)k;
  const double q0 = dk * inv_max_path;
  const double r = __builtin_fma(-(double)L.max_path(), q0, dk);
  return __builtin_fma(r, inv_max_path, q0);
}

template <int B>
__device__ __forceinline__ void shaping_lookup(const Hdr &L, double inv_max_path, const ShapeIn<B> &in,
                                               const ShapeLoads<B> &ld, ShapeQ<B> &q OC_STAMP_PARAM) {
  const int MAXP = L.max_path();
  const int completed = in.completed;
  int d_tile[B];  // min over Delivery tiles of path distance + manhattan (:382-388)
#pragma unroll
  for (int b = 0; b < B; b++) d_tile[b] = 1 << 20;
#pragma unroll
  for (int k = 0; k < OC_MAX_DELIV; k++)
    if (k < (int)L.ndeliv()) {  // uniform
#pragma unroll
      for (int b = 0; b < B; b++)
        d_tile[b] = min(d_tile[b], ld.d_tile[k][b] + manhattan(in.ap[b], (int)L.deliv_pos(k)));
    }
  // Chop term (:278-304)
  int nchop = 0;
  int mind[B];
#pragma unroll
  for (int b = 0; b < B; b++) mind[b] = 1 << 20;
#pragma unroll
  for (int f = 0; f < 3; f++)
    if (L.chop_mask(f) != 0) {  // uniform
      const int open = __popc((int)L.chop_mask(f) & ~completed);
      nchop += open;
#pragma unroll
      for (int b = 0; b < B; b++) mind[b] = open ? min(mind[b], ld.d_chop[f][b]) : mind[b];
    }
  // pair term (:319-363): agent independent
  int npairs = (int)L.pair_static_max();
  int minpair = npairs ? MAXP : (1 << 20);
  {
    int cur = MAXP;
#pragma unroll
    for (int k = 0; k < MAX_PAIRLK; k++)
      if (k < (int)L.npairlk()) {  // uniform
        cur = min(cur, ld.d_pair[k]);
        if ((L.pairlk(k) >> 8) & 1) {  // uniform: last lookup of this name pair
          const bool keep = cur != 0;    // a zero distance is not appended (:351-352)
          npairs += keep ? 1 : 0;
          minpair = keep ? min(minpair, cur) : minpair;
          cur = MAXP;
        }
      }
  }
  // the quotients
  int kq_chop[B], kq_pair;
#pragma unroll
  for (int b = 0; b < B; b++) kq_chop[b] = nchop ? (mind[b] + MAXP) + (nchop - 1) * 2 * MAXP : 0;
  kq_pair = nchop ? npairs * MAXP : (npairs ? minpair + (npairs - 1) * MAXP : 0);
  int kq_del[MAX_DELS][B];
#pragma unroll
  for (int k = 0; k < MAX_DELS; k++)
#pragma unroll
    for (int b = 0; b < B; b++) {
      kq_del[k][b] = 0;
      q.del_direct[k][b] = false;
      if (k < (int)L.ndel()) {
        const int d = ld.d_del[k][b] + manhattan(in.ap[b], in.del_p[k]);
        q.del_direct[k][b] = d == 0;                 // the agent holds it (:381)
        kq_del[k][b] = d == 0 ? d_tile[b] : d;
      }
    }
#pragma unroll
  for (int b = 0; b < B; b++) q.q_chop[b] = quotient(kq_chop[b], L, inv_max_path);
  q.q_pair = quotient(kq_pair, L, inv_max_path);
#pragma unroll
  for (int k = 0; k < MAX_DELS; k++)
#pragma unroll
    for (int b = 0; b < B; b++) q.q_del[k][b] = (k < (int)L.ndel()) ? quotient(kq_del[k][b], L, inv_max_path) : 0.0;
  q.nchop = nchop;
  q.npairs = npairs;
  OC_STAMP(4);   // distances consumed, quotients formed
}

// last third: the fp64 sums in the reference's order
template <int B>
__device__ __forceinline__ void shaping_sum(const Hdr &L, const ShapeIn<B> &in, const ShapeQ<B> &q,
                                            double &s0, double &s1 OC_STAMP_PARAM) {
  double tot[B];
#pragma unroll
  for (int b = 0; b < B; b++) {
    // `tot = 0; tot += x` of the reference is x itself (the quotients are never -0.0), so the
    // first term is selected, not added to zero
    tot[b] = q.nchop ? q.q_chop[b] : 0.0;
    tot[b] = q.npairs ? tot[b] + q.q_pair : tot[b];
  }
#pragma unroll
  for (int k = 0; k < MAX_DELS; k++)
    if (k < (int)L.ndel()) {  // uniform; Deliver term in subtask order (:370-395)
      const bool open = !((in.completed >> L.del_bit(k)) & 1);
#pragma unroll
      for (int b = 0; b < B; b++) {
        const double add = !in.del_has[k] ? 2.0 : (q.del_direct[k][b] ? q.q_del[k][b] : q.q_del[k][b] + 1.0);
        tot[b] = open ? tot[b] + add : tot[b];
      }
    }
  s0 = tot[0];
  s1 = B > 1 ? tot[1] : 0.0;
  OC_STAMP(6);   // shaping done
}

// ---------------------------------------------------------------------------
// one environment tick: OvercookedEnvironment.step
// (gym_cooking/envs/overcooked_environment.py:211-241)
// ---------------------------------------------------------------------------
// Everything up to done/reward, plus the address formation and the loads of the reward
// shaping (shaping_issue_*); the caller stores what it has to store and then calls
// shaping_lookup(L, quot, sin, sld, sq) and, after its stores, shaping_sum(L, sin, sq, ...).
// PM: arglist.play known at compile time (0 = off, 1 = on) or a run-time flag (2: R.play)
// done_p: `done` as a P word, for the callers' auto-reset selects (formed from the 0 / 1 value it is
// a compare again, and its AND with the uniform auto-reset flag a scalar read of vcc)
// FLAT: a split workgroup's arm (one duty per wave): no uniform branch in the step, see `timeout`
template <int A, int M, bool DUP, int PM, bool FLAT>
__device__ __forceinline__ void env_step(const Hdr &L, const RunCfg &R, const uint8_t *__restrict__ dist,
                                         const uint32_t *__restrict__ probe,
                                         Env<A, M, DUP> &e, const int (&act_in)[A], int &reward, int &done, P &done_p,
                                         int &success, ShapeIn<(A < 2 ? A : 2)> &sin,
                                         ShapeLoads<(A < 2 ? A : 2)> &sld OC_STAMP_PARAM) {
  const int W = L.W(), H = L.H();
  // bit k as a P word: hidden (p_bit), except in the four-way split of the general variant (PM == 2),
  // which allocates one VGPR more with the hidden form (profiles/step_prefix_ab.txt)
  const auto pb = [](int w, unsigned k) -> P {
    if constexpr (PM == 2 && FLAT) return __builtin_amdgcn_sbfe(w, k, 1u);
    return p_bit(w, k);
  };
  e.t = min(e.t + 1, 0xFFFF);  // :213 (16-bit field: saturates; max_num_timesteps <= 65535 is enforced)
  static_assert(OC_ACT_NOOP == 4 && OC_FLOOR == 0 && OC_COUNTER == 1 && OC_CUTBOARD == 2 && OC_DELIVERY == 3, "codes");

  // ---- check_collisions (:578-613) on the ORIGINAL actions -------------------
  // (per-lane predicates are P words, 0 / -1: see `hide`)
  int act[A], np[A], tgt_p[A];   // action, proposed cell, interact()'s target cell
  P moving[A], t_nonfloor[A], t_deliv[A], t_cutb[A];   // action != (0,0); tile type of the target cell
#pragma unroll
  for (int a = 0; a < A; a++) {
    int c = act_in[a];
    e.err |= p_gtu_any((unsigned)c, 4u) & OC_ERR_ACTION;   // no such NAV action: flagged, executed as (0, 0)
    c = (int)min((unsigned)c, 4u);
    act[a] = c;
    moving[a] = p_ne(c, OC_ACT_NOOP);
    int cell;   // dense index of the target cell
    P oob = 0;
    if constexpr (OC_BORDER_CLOSED) {
      // packed cell += {+16, -16, -1, +1, 0}: one signed byte per action code
      constexpr uint64_t STEP = 0x0001FFF010ull;  // NOOP 00 | RIGHT 01 | LEFT ff | UP f0 | DOWN 10
      const int q = e.ap[a] + (int)(int8_t)(STEP >> (8 * c));
      tgt_p[a] = q;
      cell = dense(L, q);
    } else {
      const int dx = (c == OC_ACT_RIGHT) - (c == OC_ACT_LEFT);
      const int dy = (c == OC_ACT_DOWN) - (c == OC_ACT_UP);
      const int qx = px(e.ap[a]) + dx, qy = py(e.ap[a]) + dy;
      oob = ~(p_ltu_any((unsigned)qx, (unsigned)W) & p_ltu_any((unsigned)qy, (unsigned)H));
      e.err |= oob & OC_ERR_OOB;  // get_gridsquare_at asserts (utils/world.py:310-315)
      const int tx = min(max(qx, 0), W - 1), ty = min(max(qy, 0), H - 1);  // world.inbounds (world.py:317-320)
      tgt_p[a] = tx | (ty << 4);
      cell = ty * W + tx;
    }
    // tile type of the target cell as three predicates, straight from the bit-planes
    P lo, hi;
    if (!L.planes128()) {   // uniform (compile-time in specialised builds)
      lo = pb((int)(L.cell_lo(0) >> cell), 0);
      hi = pb((int)(L.cell_hi(0) >> cell), 0);
    } else {
      lo = -bit128(L.cell_lo(0), L.cell_lo(1), cell);
      hi = -bit128(L.cell_hi(0), L.cell_hi(1), cell);
    }
    t_nonfloor[a] = lo | hi;
    t_deliv[a] = lo & hi;
    t_cutb[a] = hi & ~lo;
    np[a] = sel(t_nonfloor[a] | oob, e.ap[a], tgt_p[a]);  // :551-559
  }
  P ex[A];
#pragma unroll
  for (int a = 0; a < A; a++) ex[a] = -1;
#pragma unroll
  for (int i = 0; i < A; i++)
#pragma unroll
    for (int j = i + 1; j < A; j++) {
      const P same = p_eq(np[i], np[j]);  // :562-569
      const P i_stays = p_eq(np[i], e.ap[i]) & moving[i];
      const P j_stays = p_eq(np[j], e.ap[j]) & moving[j];
      const P swap = p_eq(e.ap[i], np[j]) & p_eq(e.ap[j], np[i]);  // :572-575
      const P block_i = sel(same, ~i_stays, swap);
      const P block_j = sel(same, i_stays | ~j_stays, swap);
      ex[i] &= ~block_i;
      ex[j] &= ~block_j;
    }

  // ---- execute_navigation (:615-618): interact(), sequential in agent order ---
  // decision phase + one bit-field insert per item (utils/interact.py:4-75)
  // arglist.play (uniform): a merge is put straight onto the counter (:44-47), a fresh food is
  // put DOWN on a Cutboard (:52) and chopped where it lies by an empty-handed press (:66-67)
  const P play = p_of(PM == 2 ? R.play != 0 : PM == 1);
#pragma unroll
  for (int a = 0; a < A; a++) {
    const P acting = ex[a] & moving[a];  // blocked -> (0,0) (:610-612); interact.py:12
    // the agent's own cell has not changed since the proposal phase (only its own interact()
    // moves it), so the target cell and its tile type computed there still hold
    const int pa = e.ap[a];
    const int tp = tgt_p[a];
    // held group (ahp - 1; -1 = empty hands): its sign is "not holding", and the subtraction is the
    // one `newg` needs anyway (p_nz(ahp) on the extracted field came out as a carry into vcc + select)
    // (two agents only: in the three- and four-agent kernels this form allocates one to two VGPRs more)
    const int held_g = A == 2 ? hide(e.ahp[a] - 1) : e.ahp[a] - 1;
    const P holding = A == 2 ? ~hide(held_g >> 31) : p_nz(e.ahp[a]);
    const int hold_code = (a + 1) << 12;
    // the held Object (items with holder == a) and the unheld Object on the target cell, as
    // ORs of their item words with bit 8 turned into "a food that is still fresh"
    int held_or = 0, tgt_or = 0;
    P mine[M], tgt[M];
#pragma unroll
    for (int i = 0; i < M; i++) {
      const int w = e.iw[i];
      const int u = item_type(L, i) != OC_PLATE ? (w ^ IW_CHOP) : w;  // uniform choice; a Plate is never chopped
      // (two agents: holder + 1 is 0, 1 or 2, so "held by agent a" is ONE bit of the word)
      mine[i] = A == 2 ? pb(w, 12 + a) : p_eq(w & IW_HOLD, hold_code);
      tgt[i] = p_eq(w & (IW_HOLD | IW_POS), tp);                       // unheld and on the target cell
      held_or |= mine[i] & u;
      tgt_or |= tgt[i] & u;
    }
    const P tgt_any = p_nz(tgt_or);                                     // tset of an item is never empty
    P held_multi;                                                       // > 1 content
    if constexpr (DUP) {   // counts: two of one type are two contents
      int nm = 0;
#pragma unroll
      for (int i = 0; i < M; i++) nm -= mine[i];
      held_multi = p_gt(nm, 1);
    } else {
      held_multi = p_nz(held_or & IW_TSET & ((held_or & IW_TSET) - (1 << 24)));
    }
    const P held_fresh = pb(held_or, 8);
    const P any_fresh = pb(held_or | tgt_or, 8);
    const P two_plates = p_nz((held_or & tgt_or) & sig_of_type<DUP>(OC_PLATE));
    const P at_deliv = t_deliv[a];
    const P nf = acting & t_nonfloor[a];
    const P do_move = acting & ~t_nonfloor[a];                                        // interact.py:19-20
    const P nfh = nf & holding & ~at_deliv, nfe = nf & ~holding & ~at_deliv;
    const P do_deliver = nf & holding & at_deliv & held_multi & ~held_fresh;          // :25-30, core.py:232-237
    const P mergeable = ~(two_plates | any_fresh);                                    // core.py:240-257
    const P do_merge = nfh & tgt_any & mergeable;                                     // :33-46
    const P chop_here = t_cutb[a] & ~held_multi & held_fresh & ~play;                 // :52
    const P do_chop = nfh & ~tgt_any & chop_here;                                     // :52-54
    const P do_drop = nfh & ~tgt_any & ~chop_here;                                    // :56-57
    const P chop_there = nfe & tgt_any & play & t_cutb[a] & pb(tgt_or, 8);         // :66-67 (a fresh food is always alone)
    const P do_pick = nfe & tgt_any & ~chop_there & p_of(!((R.allergic >> a) & 1));   // :62-71, agent.py:296-298
    const P put = do_deliver | do_drop | (do_merge & play);
    const P take = (do_merge & ~play) | do_pick;
    // min(held group, or 7 with empty hands; group on the target cell): -1 is the largest unsigned
    const int newg = (int)min((unsigned)held_g, (unsigned)igrp(tgt_or));  // only used when `take` (then tgt_any)
    // the merged Object: smallest item id as group, re-inserted under a new name = last in
    // world order (world.py:236-237), union of the type sets
    int objf;
    if constexpr (DUP) {
      // the merged name = the two multisets added; its key rank: looked up / entered in the
      // per-env name table (see Env::kn)
      const int newsig = (held_or & TS<true>) + (tgt_or & TS<true>);
      const int seq4 = M + e.mctr;
      int kf = 0;
#pragma unroll
      for (int j = 0; j < MAX_NAMES; j++)
        if (j < (int)L.nnames()) {   // uniform
          const P hit = p_eq(newsig >> 24, (int)L.name_sig(j));
          const int sh = 4 * (j & 7);
          const int cur = (e.kn[j >> 3] >> sh) & 15;
          kf = sel(hit, cur, kf);
          const P enter = hit & p_z(cur);   // first Object of this name this episode: the key is created now
          e.kn[j >> 3] |= enter & do_merge & ((seq4 + 1) << sh);
        }
      const int kseq = sel(p_nz(kf), kf - 1, seq4);
      objf = newsig | (newg << 9) | (((kseq << 4) | seq4) << 16);
    } else {
      objf = ((held_or | tgt_or) & IW_TSET) | (newg << 9) | ((M + e.mctr) << 16);
    }
    if (A > 2) {
      // World.remove(agent.holding) deletes by (name, location), last match
      // (world.py:239-247): with another agent on the same cell holding a same-named
      // Object that sits later in world order it removes the wrong one and the
      // reference's store is corrupt from here on.  Flag it.
      // Only reachable when another agent stands on this agent's cell (the 3-agent overlap
      // quirk of check_collisions) while this one merges: one ballot skips the item scan for
      // the whole wave in every other step.
      // (Tried: ONE ballot per step on "two agents may come to share a cell" -- any pair with equal
      // old or proposed cells -- instead of one per agent: true in nearly every wave of 64 three-agent
      // envs, so the scan below ran always: tl-3 x 65 536 3.82 -> 4.16 us.  The ballot per agent costs
      // a scalar read of a vector-written mask, ~16 cycles, and is almost never taken.)
      P shared = 0;
#pragma unroll
      for (int b = 0; b < A; b++)
        if (b != a) shared |= p_eq(e.ap[b], pa);
      if (__ballot((shared & do_merge) != 0) != 0) {
        P alias = 0;
#pragma unroll
        for (int j = 0; j < M; j++) {
          const int w = e.iw[j];
          alias |= p_nz(w & IW_HOLD) & p_ne(w & IW_HOLD, hold_code) & p_eq(ipos(w), pa) &
                   p_z((w ^ held_or) & TS<DUP>) & p_gt(w & IW_SEQ, held_or & IW_SEQ);
        }
        e.err |= shared & do_merge & alias & OC_ERR_ALIAS;
      }
    }
    // held items: cell <- target (move / put down), holder <- none (put down), object
    // fields (merge), chopped (chop); target-cell items: cell <- agent, holder <- agent
    // (merge / pick up), object fields (merge)
    const int mask_m = ((do_move | put) & IW_POS) | (put & IW_HOLD) | (do_merge & OBJ<DUP>) | (do_chop & IW_CHOP);
    const int mask_t = (take & (IW_POS | IW_HOLD)) | (do_merge & OBJ<DUP>) | (chop_there & IW_CHOP);
    const int val_m = tp | IW_CHOP | objf;
    const int val_t = pa | hold_code | objf | IW_CHOP;
#pragma unroll
    for (int i = 0; i < M; i++) {
      // (an item is held by this agent or lies unheld on the target cell, never both)
      const int selm = (mine[i] & mask_m) | (tgt[i] & mask_t);
      e.iw[i] = bfi(selm, sel(mine[i], val_m, val_t), e.iw[i]);
    }
    e.ap[a] = sel(do_move, tp, pa);  // agent.py:311-314
    e.ahp[a] = sel(take, newg + 1, e.ahp[a]) & ~put;
    e.mctr -= do_merge;
  }

  // ---- calculate_reward_shaping (:272-397): the position-only distance lookups go out now ----
  constexpr int B = A < 2 ? A : 2;
#pragma unroll
  for (int b = 0; b < B; b++) sin.ap[b] = e.ap[b];
  if constexpr (DUP) {
    // Chop(X): get_all_object_locs(fresh X)[0] (:287) -- with two fresh X, the set's element [0]
#pragma unroll
    for (int f = 0; f < 3; f++) {
      sin.chop_p[f] = 0;
      if (L.chop_mask(f) != 0) {   // uniform
        bool cand[M];
#pragma unroll
        for (int i = 0; i < M; i++) cand[i] = ((L.food_items(f) >> i) & 1) && !(e.iw[i] & IW_CHOP);
        int has;
        sin.chop_p[f] = pyset_first<M>(L, probe, e.iw, cand, has);
      }
    }
  }
  {
    int ipb[M];
#pragma unroll
    for (int i = 0; i < M; i++) ipb[i] = ipos(e.iw[i]);
    shaping_issue_pos<B, M, DUP>(L, dist, sin, ipb, sld);
    // keep the lookups HERE: left alone, the scheduler sinks them below done/reward, ~40
    // instructions ahead of their first use
    __builtin_amdgcn_sched_barrier(0);
  }
  OC_STAMP(2);
  // ---- done (:243-270) and reward (:399-432) ---------------------------------
  // present / at_delivery: bit s set iff an Object with type-set s and every food chopped
  // exists (anywhere / on the first Delivery tile).  A multi-item Object is all-chopped
  // by construction (mergeable() required it).
  const int d0 = (int)L.deliv_pos(0);  // first Delivery tile only (:259,:402)
  int present = 0, at_delivery = 0;
  P rep_ok[M];   // item i represents its Object (group == i) and the Object is all-chopped
#pragma unroll
  for (int i = 0; i < M; i++) {
    const int w = e.iw[i];
    const P rep = p_eq(w & IW_GRP, i << 9);
    // a lone fresh food is the only Object that is not all-chopped
    const P lone_fresh = item_type(L, i) != OC_PLATE   // uniform
                             ? p_eq(w & (TS<DUP> | IW_CHOP), sig_of_type<DUP>(item_type(L, i))) : 0;
    rep_ok[i] = rep & ~lone_fresh;
    if constexpr (!DUP) {
      const int b = rep_ok[i] & (1 << itset(w));
      present |= b;
      at_delivery |= p_eq(ipos(w), d0) & b;
    }
  }
  int cnt_mask = 0, del_mask = 0, newly;
  if constexpr (DUP) {
    // a goal object may exist several times: its count = the number of DISTINCT cells that hold
    // one (get_all_object_locs is a set of locations, world.py:290-291), two bits per goal
    int rose = 0;
#pragma unroll
    for (int g = 0; g < MAX_GOALS; g++)
      if (g < (int)L.ngoal()) {  // uniform
        int cnt = 0;
        P hasd = 0;
        P m[M];
#pragma unroll
        for (int i = 0; i < M; i++) {
          m[i] = rep_ok[i] & p_eq(e.iw[i] & TS<true>, (int)L.goal_sig(g) << 24);
          P seen = 0;
#pragma unroll
          for (int j = 0; j < i; j++) seen |= m[j] & p_eq(ipos(e.iw[j]), ipos(e.iw[i]));
          cnt -= m[i] & ~seen;
          hasd |= m[i] & p_eq(ipos(e.iw[i]), d0);
        }
        cnt = min(cnt, 3);
        const int old = (e.goalcnt >> (2 * g)) & 3;
        rose |= p_gt(cnt, old) & (int)L.goal_nd(g);
        cnt_mask |= cnt << (2 * g);
        del_mask |= hasd & (int)L.goal_dl(g);
      }
    newly = rose;
  } else {
#pragma unroll
    for (int g = 0; g < MAX_GOALS; g++) {
      if (g < (int)L.ngoal()) {  // uniform
        cnt_mask |= pb(present, L.goal_tset(g)) & (int)L.goal_nd(g);
        del_mask |= pb(at_delivery, L.goal_tset(g)) & (int)L.goal_dl(g);
      }
    }
    newly = cnt_mask & ~e.goalcnt;  // goal count rose above goal_objects_count (:408-415)
  }
  reward = __popc(newly) + 3 * __popc(del_mask);  // Deliver pays +3 every step (:400-406)
  e.completed |= newly | del_mask;
  e.goalcnt = cnt_mask;
  // checked first (:245-249).  No limit (T == 0, uniform): FLAT, compared with a value t never
  // reaches (t is a 16-bit field) -- a uniform select of the operand, no branch round the compare.
  // The one-wave kernels keep the branch: without it their code up to the first store is one
  // scheduling region, and they allocate 2 to 4 VGPRs more (profiles/step_prefix_ab.txt).
  P timeout;
  if constexpr (FLAT) timeout = p_ge(e.t, R.T != 0 ? (int)R.T : 0x10000);
  else timeout = R.T != 0 ? p_ge(e.t, R.T) : 0;
  const P all_delivered = p_eq_any(del_mask, (int)L.deliver_mask());   // (32-bit subtask masks)
  done_p = hide(timeout | all_delivered);
  done = done_p & 1;
  success = (~timeout & all_delivered) & 1;

  // ---- calculate_reward_shaping for sim agents 0 and 1 (:272-397): the rest of the inputs ----
  sin.completed = e.completed;
#pragma unroll
  for (int k = 0; k < MAX_DELS; k++) {
    sin.del_has[k] = 0;
    sin.del_p[k] = 0;
    if (k < (int)L.ndel()) {  // uniform
      if constexpr (DUP) {   // get_all_object_locs(goal object)[0] (:374-379): the set's element [0]
        bool cand[M];
#pragma unroll
        for (int i = 0; i < M; i++)
          cand[i] = (rep_ok[i] & p_eq(e.iw[i] & TS<true>, (int)L.del_sig(k) << 24)) != 0;
        sin.del_p[k] = pyset_first<M>(L, probe, e.iw, cand, sin.del_has[k]);
      } else {
#pragma unroll
        for (int i = 0; i < M; i++) {
          const P ok = rep_ok[i] & p_eq(e.iw[i] & IW_TSET, (int)L.del_tset(k) << 24);
          sin.del_has[k] |= ok & 1;
          sin.del_p[k] = sel(ok, ipos(e.iw[i]), sin.del_p[k]);
        }
      }
    }
  }
  shaping_issue_del<B>(L, dist, sin, sld);
  __builtin_amdgcn_sched_barrier(0);   // ... and these ahead of the caller's stores
  OC_STAMP(3);   // done/reward computed, distance loads issued
}

// get_observation2 (gym_comm/envs/overcooked_env.py:105-159) for one viewer;
// writes F = 22 + S + 2C rows with stride n.
// OT = element type of the observation rows: 0 int32, 1 int8, 2 float32 (the same integers,
// converted; what a policy network's first layer consumes as obs[v].T without a cast)
// The bit of `completed` that each completed_subtasks row shows (RunCfg::slot4), one scalar per
// row: it depends on the launch alone, so a caller with idle time before its stores forms it there
// (multi_step_body: in front of the barrier) and the rows themselves are one bit-field extract each,
// with no test of slot_identity among the stores.  Specialised builds only (S is a constant).
#ifdef OC_SPECIALIZED
constexpr int OBS_NSLOT = OC_SPEC_HDR.S > 0 ? OC_SPEC_HDR.S : 1;
#else
constexpr int OBS_NSLOT = 1;
#endif
struct ObsSlots {
  int sh[OBS_NSLOT];
  __device__ __forceinline__ ObsSlots(const RunCfg &R, bool pin) {
#ifdef OC_SPECIALIZED
#pragma unroll
    for (int s = 0; s < (int)OC_SPEC_HDR.S; s++) {
      sh[s] = R.slot_identity ? s : (int)((R.slot4[s >> 2] >> (8 * (s & 3))) & 31);   // uniform
      if (pin) asm volatile("" : "+s"(sh[s]));
    }
#else
    sh[0] = 0;
#endif
  }
};

template <int A, int M, bool DUP, int OT, typename OutRows>
__device__ __forceinline__ void env_obs(const Hdr &L, const RunCfg &R, const ObsSlots &slots, const Env<A, M, DUP> &e,
                                        int viewer, int radius, bool viewer_blind, bool ego_blind, int C, int comm0,
                                        int comm1, const OutRows &out, int row0) {
  const int vp = viewer == 0 ? e.ap[0] : e.ap[1];
  const int vhp = viewer == 0 ? e.ahp[0] : e.ahp[1];
  const int vx = px(vp), vy = py(vp);
  int ddx[4], ddy[4], st[4], hid[4];
  int loc[4];   // agent1_location, agent2_location
  if (viewer_blind) {  // uniform: deltas and locations 0, everything hidden (:109,:139-143)
#pragma unroll
    for (int ch = 0; ch < 4; ch++) ddx[ch] = ddy[ch] = st[ch] = loc[ch] = 0, hid[ch] = 1;
  } else {
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
      // last writer in world.objects order wins (:121-131): the item of this type
      // whose Object has the highest rank
      int bw = 0;
      bool any = false;
#pragma unroll
      for (int i = 0; i < M; i++)
        if (item_type(L, i) == ch) {  // uniform
          bw = (!any || (e.iw[i] & IW_SEQ) > (bw & IW_SEQ)) ? e.iw[i] : bw;
          any = true;
        }
      // an absent type keeps delta (0,0)
      const int bx = any ? px(ipos(bw)) : vx, by = any ? py(ipos(bw)) : vy;
      const bool within = (int)sad_u32(bx, vx, sad_u32(by, vy, 0u)) <= radius;   // |dx| + |dy|
      hid[ch] = within ? 0 : 1;                       // :133
      ddx[ch] = within ? 0 : bx - vx;                 // :135 (sic: zeroed when visible)
      ddy[ch] = within ? 0 : by - vy;
      st[ch] = (any && ch != OC_PLATE) ? ichop(bw) : 0;
    }
    loc[0] = px(e.ap[0]), loc[1] = py(e.ap[0]), loc[2] = px(e.ap[1]), loc[3] = py(e.ap[1]);
  }
#define OUT(r_, v_)                                                              \
  do {                                                                           \
    if (OT == 1) out.st8((r_), (v_));                                            \
    else if (OT == 2) out.st((r_), __builtin_bit_cast(int, (float)(v_)));        \
    else out.st((r_), (v_));                                                     \
  } while (0)
  int row = row0;
#pragma unroll
  for (int ch = 0; ch < 4; ch++) OUT(row++, ddx[ch]);
#pragma unroll
  for (int ch = 0; ch < 4; ch++) OUT(row++, ddy[ch]);
#pragma unroll
  for (int ch = 0; ch < 4; ch++) OUT(row++, st[ch]);
#pragma unroll
  for (int ch = 0; ch < 4; ch++) OUT(row++, hid[ch]);
  // (a run of rows whose number is only known at run time: the byte offset is carried along)
#define OUT_AT(so_, r_, v_)                                                            \
  do {                                                                                 \
    if (OT == 1) out.st8_at((so_), (r_), (v_));                                        \
    else if (OT == 2) out.st_at((so_), (r_), __builtin_bit_cast(int, (float)(v_)));    \
    else out.st_at((so_), (r_), (v_));                                                 \
  } while (0)
#ifdef OC_SPECIALIZED
#pragma unroll
  for (int s = 0; s < (int)OC_SPEC_HDR.S; s++) OUT(row++, (e.completed >> slots.sh[s]) & 1);
#else
  {
    int so = out.soff(row);
    if (R.slot_identity) {   // uniform: the caller's order is the canonical one
      for (int s = 0; s < L.S(); s++, row++, so += out.rowbytes) OUT_AT(so, row, (e.completed >> s) & 1);
    } else {
      for (int s = 0; s < L.S(); s++, row++, so += out.rowbytes)
        OUT_AT(so, row, (e.completed >> ((R.slot4[s >> 2] >> (8 * (s & 3))) & 31)) & 1);
    }
  }
#endif
#pragma unroll
  for (int k = 0; k < 4; k++) OUT(row++, loc[k]);
  OUT(row++, ego_blind ? 0 : (vhp != 0 ? 1 : 0));  // :154, gated on the EGO's BLIND flag
  OUT(row++, 0);
  // comm one-hots: straight-line for up to four channels (uniform switch; the BASELINE
  // configuration has two), a loop beyond.  (Every case ends on an empty asm statement: the
  // optimiser otherwise merges the cases' last stores into one shared tail and pays for it with
  // a dozen flag moves and branches -- inline asm is never sunk into a common successor.)
#define COMM_ROWS(CC_)                                                     \
  do {                                                                     \
    _Pragma("unroll") for (int c = 0; c < (CC_); c++) OUT(row + c, comm0 == c ? 1 : 0);          \
    _Pragma("unroll") for (int c = 0; c < (CC_); c++) OUT(row + (CC_) + c, comm1 == c ? 1 : 0);  \
    asm volatile("");                                                                            \
  } while (0)
  if (C == 2) {   // the BASELINE configuration first: one compare and one branch ...
    COMM_ROWS(2);
  } else {
    int Cx = C;
    asm("" : "+s"(Cx));   // (... which the optimiser would otherwise fold back into the switch)
    switch (Cx) {
      case 1: COMM_ROWS(1); break;
      case 3: COMM_ROWS(3); break;
      case 4: COMM_ROWS(4); break;
      default: {
        int so = out.soff(row);
        for (int c = 0; c < C; c++, row++, so += out.rowbytes) OUT_AT(so, row, comm0 == c ? 1 : 0);
        for (int c = 0; c < C; c++, row++, so += out.rowbytes) OUT_AT(so, row, comm1 == c ? 1 : 0);
      }
    }
  }
#undef COMM_ROWS
#undef OUT_AT
#undef OUT
}

#ifdef OC_SPECIALIZED
// LANE-SPLIT launch (k_multi_step<..., LN = 2>; four lanes per env were built, measured slower at
// every batch size and taken out again): an env has LN lanes of every wave -- lane l of
// the wave serves env (l mod 64/LN) of the workgroup as PART l / (64/LN) -- and the parts of an env
// produce DIFFERENT observation rows with the SAME instructions: the row of a part lies a constant
// number of rows behind part 0's, so the distance is added once, per lane, to the byte offset the
// store takes anyway, and one row store writes LN rows.  What a part needs of the launch alone is
// formed here, by the observation waves, under the wait for the state:
//   voA  channel rows (ddx / ddy / st / hid) and the agent locations: part p takes the 4 / LN
//        channels (location words) from p * 4 / LN on, i.e. rows 4 / LN apart
//   vo1  rows paired at distance 1 (subtask bits two by two, holding + the zero row)
//   voC  the comm one-hots, comm1[c] C rows behind comm0[c]
//   hi   the part as a P word (0 / -1), shp[k] the bit of `completed` that subtask row 2 k (part 1:
//        2 k + 1) shows
template <int LN>
struct LaneParts {
  static_assert(LN == 2, "lanes per env");
  static constexpr int NPAIR = (int)OC_SPEC_HDR.S / 2;
  int voA, vo1, voC;
  P hi;
  int shp[NPAIR > 0 ? NPAIR : 1];
  int sh_odd;   // (uniform) the bit an odd last subtask row shows: stored by every part
  template <int AUX>
  __device__ __forceinline__ LaneParts(const RowsT<AUX> &ob, const ObsSlots &slots, int C) {
    const int tid = (int)threadIdx.x;
    hi = p_bit(tid, 5);
    voA = ob.voff + (hi & ((4 / LN) * ob.rowbytes));
    vo1 = ob.voff + (hi & ob.rowbytes);
    voC = ob.voff + (hi & (C * ob.rowbytes));
    asm volatile("" : "+v"(voA), "+v"(vo1), "+v"(voC), "+v"(hi));   // formed HERE, like RowsPreT's offsets
#pragma unroll
    for (int k = 0; k < NPAIR; k++) {
      shp[k] = sel(hi, slots.sh[2 * k + 1], slots.sh[2 * k]);
      asm volatile("" : "+v"(shp[k]));
    }
    sh_odd = (OC_SPEC_HDR.S & 1) ? slots.sh[OBS_NSLOT - 1] : 0;
  }
  // the value of this lane's part among one per part
  __device__ __forceinline__ int pick(const int (&v)[LN]) const { return sel(hi, v[1], v[0]); }
};

struct NoParts {   // (what a wave that is not a lane-split observation wave holds instead)
  template <typename... T>
  __device__ __forceinline__ NoParts(const T &...) {}
};

// env_obs for one part of a lane-split launch: the plain variant's configuration (nobody BLIND),
// the same rows with the same values -- each stored by the part LaneParts names, the rest (an odd
// subtask row, the comm rows of more than four channels, the timestep by the caller) by every
// part alike: the same value to the same address.
template <int A, int M, bool DUP, int OT, int LN, typename OutRows>
__device__ __forceinline__ void env_obs_lanes(const Hdr &L, const LaneParts<LN> &lp, const Env<A, M, DUP> &e,
                                              int viewer, int radius, int C, int comm0, int comm1,
                                              const OutRows &out, int row0) {
  constexpr int CPP = 4 / LN;   // channels (location words) per part
  constexpr int S = (int)OC_SPEC_HDR.S;
  const int vp = viewer == 0 ? e.ap[0] : e.ap[1];
  const int vhp = viewer == 0 ? e.ahp[0] : e.ahp[1];
  const int vx = px(vp), vy = py(vp);
  const int loc4[4] = {px(e.ap[0]), py(e.ap[0]), px(e.ap[1]), py(e.ap[1])};
  int ddx[CPP], ddy[CPP], st[CPP], hid[CPP], loc[CPP];
#pragma unroll
  for (int j = 0; j < CPP; j++) {
    // channel q * CPP + j in part q: its winning item word (see env_obs), selected BEFORE the
    // arithmetic all parts share
    int bwq[LN], anyq[LN], chopq[LN], locq[LN];
#pragma unroll
    for (int q = 0; q < LN; q++) {
      const int ch = q * CPP + j;
      int bw = 0;
      bool any = false;
#pragma unroll
      for (int i = 0; i < M; i++)
        if (item_type(L, i) == ch) {  // uniform
          bw = (!any || (e.iw[i] & IW_SEQ) > (bw & IW_SEQ)) ? e.iw[i] : bw;
          any = true;
        }
      bwq[q] = bw;
      anyq[q] = any ? -1 : 0;
      chopq[q] = (any && ch != OC_PLATE) ? 1 : 0;
      locq[q] = loc4[ch];
    }
    const int bw = lp.pick(bwq);
    const P any = lp.pick(anyq);
    const int bx = sel(any, px(ipos(bw)), vx), by = sel(any, py(ipos(bw)), vy);   // an absent type keeps delta (0,0)
    const bool within = (int)sad_u32(bx, vx, sad_u32(by, vy, 0u)) <= radius;
    hid[j] = within ? 0 : 1;
    ddx[j] = within ? 0 : bx - vx;
    ddy[j] = within ? 0 : by - vy;
    st[j] = ichop(bw) & lp.pick(chopq);
    loc[j] = lp.pick(locq);
  }
#define OUTV(r_, vo_, v_)                                                               \
  do {                                                                                  \
    if (OT == 1) out.st8_v((r_), (vo_), (v_));                                          \
    else if (OT == 2) out.st_v((r_), (vo_), __builtin_bit_cast(int, (float)(v_)));      \
    else out.st_v((r_), (vo_), (v_));                                                   \
  } while (0)
  int row = row0;
#pragma unroll
  for (int j = 0; j < CPP; j++) OUTV(row + j, lp.voA, ddx[j]);
#pragma unroll
  for (int j = 0; j < CPP; j++) OUTV(row + 4 + j, lp.voA, ddy[j]);
#pragma unroll
  for (int j = 0; j < CPP; j++) OUTV(row + 8 + j, lp.voA, st[j]);
#pragma unroll
  for (int j = 0; j < CPP; j++) OUTV(row + 12 + j, lp.voA, hid[j]);
  row += 16;
#pragma unroll
  for (int k = 0; k < S / 2; k++) OUTV(row + 2 * k, lp.vo1, (e.completed >> lp.shp[k]) & 1);
  if constexpr ((S & 1) != 0) OUTV(row + S - 1, out.voff, (e.completed >> lp.sh_odd) & 1);
  row += S;
#pragma unroll
  for (int j = 0; j < CPP; j++) OUTV(row + j, lp.voA, loc[j]);
  row += 4;
  OUTV(row, lp.vo1, p_nz(vhp) & ~lp.hi & 1);   // holding | the zero row behind it
  row += 2;
  const int commv = sel(lp.hi, comm1, comm0);
#define COMM_ROWS(CC_)                                                                              \
  do {                                                                                              \
    _Pragma("unroll") for (int c = 0; c < (CC_); c++) OUTV(row + c, lp.voC, commv == c ? 1 : 0);   \
    asm volatile("");                                                                               \
  } while (0)
  if (C == 2) {
    COMM_ROWS(2);
  } else {
    int Cx = C;
    asm("" : "+s"(Cx));
    switch (Cx) {
      case 1: COMM_ROWS(1); break;
      case 3: COMM_ROWS(3); break;
      case 4: COMM_ROWS(4); break;
      default: {   // the loop stays unsplit
        int so = out.soff(row);
        for (int c = 0; c < C; c++, row++, so += out.rowbytes) {
          if (OT == 1) out.st8_at(so, row, comm0 == c ? 1 : 0);
          else if (OT == 2) out.st_at(so, row, __builtin_bit_cast(int, (float)(comm0 == c ? 1 : 0)));
          else out.st_at(so, row, comm0 == c ? 1 : 0);
        }
        for (int c = 0; c < C; c++, row++, so += out.rowbytes) {
          if (OT == 1) out.st8_at(so, row, comm1 == c ? 1 : 0);
          else if (OT == 2) out.st_at(so, row, __builtin_bit_cast(int, (float)(comm1 == c ? 1 : 0)));
          else out.st_at(so, row, comm1 == c ? 1 : 0);
        }
      }
    }
  }
#undef COMM_ROWS
#undef OUTV
}
#endif

// Sum of a per-lane integer over the 64 lanes of the wave, left in lane 63: an inclusive scan
// inside each row of 16 lanes (row_shr 1/2/4/8, zero fill), then row 0 -> 1, 2 -> 3
// (row_bcast:15) and rows 0-1 -> 2-3 (row_bcast:31).  Six DPP adds, no LDS, no SALU loop.
__device__ __forceinline__ int wave_sum_lane63(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);   // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);   // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);   // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);   // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);  // row_bcast:15 into rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);  // row_bcast:31 into rows 2, 3
  return v;
}

// Per-wave metric accumulation: the six counters of a step are packed into two words per
// lane (every field wide enough for a sum over 64 lanes), both words are summed across the
// wave with DPP adds, the totals are read from lane 63 into SGPRs, split by scalar bit-field
// extracts and written back into lanes 0..5, and lane k adds counter k to the wave's OWN
// 64-byte slot of the metrics tensor (one no-return atomic per lane, no two waves share a
// slot).  Must be called with all 64 lanes active.
struct MetricsSlot {
  unsigned long long *p;
  // thread_index: global thread id; one slot per 64 envs
  __device__ __forceinline__ MetricsSlot(int64_t *metrics, int64_t thread_index) {
    const int lane = threadIdx.x & 63;
    p = (metrics != nullptr && lane < 6)
            ? (unsigned long long *)metrics + (thread_index >> 6) * OC_MET_COUNT + lane
            : nullptr;
  }
  __device__ __forceinline__ void add(bool has_metrics, bool valid, int done, int success, int reward,
                                      int completed_bits, bool err) {
    if (!has_metrics) return;  // uniform
    // (P words, see `hide`: valid / done / success / err combine on the vector unit)
    const P ok = hide(valid ? -1 : 0), fin = ok & -done;
    // word A: reward (<= 32 + 3 * MAX_DELS < 64 -> 12-bit sum) | completed subtasks of a finished
    // episode (<= OC_MAX_SUBTASKS = 32 per lane, 64 lanes -> a 12-bit sum)
    // word B: valid | done | success | error, 7 bits each (a count up to 64)
    const int a = (ok & reward) | ((fin & __popc(completed_bits)) << 12);
    const int b = (ok & 1) | (fin & (1 << 7)) | (ok & -success & (1 << 14)) | (ok & hide(err ? -1 : 0) & (1 << 21));
    const unsigned ta = (unsigned)__builtin_amdgcn_readlane(wave_sum_lane63(a), 63);
    const unsigned tb = (unsigned)__builtin_amdgcn_readlane(wave_sum_lane63(b), 63);
    // lane k picks counter k out of the two totals: a per-lane (word, offset, width) from
    // three packed constants -- plain VALU selects, no divergent control flow
    constexpr unsigned OFF = 0u | 7u << 5 | 14u << 10 | 0u << 15 | 12u << 20 | 21u << 25;    // 5 bits per lane
    constexpr unsigned WID = 7u | 7u << 5 | 7u << 10 | 12u << 15 | 12u << 20 | 7u << 25;
    static_assert(64 * OC_MAX_SUBTASKS < (1 << 12) && 64 * (OC_MAX_SUBTASKS + 3 * MAX_DELS) < (1 << 12),
                  "wave sums must fit their 12-bit fields");
    static_assert(OC_MET_ENV_STEPS == 0 && OC_MET_EPISODES == 1 && OC_MET_SUCCESSES == 2 &&
                  OC_MET_REWARD_SUM == 3 && OC_MET_COMPLETED_SUM == 4 && OC_MET_ERRORS == 5, "slot order");
    const unsigned lane = threadIdx.x & 63, k5 = (lane < 6 ? lane : 0) * 5;
    const unsigned off = (OFF >> k5) & 31, wid = (WID >> k5) & 31;
    const unsigned src = (lane == OC_MET_REWARD_SUM || lane == OC_MET_COMPLETED_SUM) ? ta : tb;
    const int v = (int)((src >> off) & ((1u << wid) - 1u));
    // Fire-and-forget atomic add by lanes 0..5, each to its own word of the wave's OWN slot (no
    // contention).  A load at kernel start + a plain store here had to be consumed behind the
    // 60+ stores of the step: vmcnt retires in issue order, so the wave ended on an
    // s_waitcnt vmcnt(0) -- a wait for every store it had issued.
    if (p) __hip_atomic_fetch_add(p, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
};

// ---------------------------------------------------------------------------
// kernels
// ---------------------------------------------------------------------------
// The two lane-indexed tables (fp64 quotients, then the u8 distance table) sit in one
// device buffer.  Two variants of every step kernel exist (template bool LDS):
//   LDS = false  the tables are read straight from global memory (vector L1/L2): no
//                staging pass, no barrier.  The default: fastest at every batch size with
//                64- or 128-thread workgroups (round-1 v3 sweep: n = 4096: 4.7 us vs
//                5.7 us per step; n = 131072: 11.1 us vs 12.7 us).
//   LDS = true   every workgroup copies them to LDS with 16-byte loads issued BEFORE the
//                state loads, so both round trips overlap.  Only ahead with 256-thread
//                workgroups (n = 131072: 12.1 us vs 13.3 us), which lose overall.
// Full sweep: profiles/r01_v3_block_lds_sweep.txt.
struct Tables {
  const uint8_t *dist;
  const uint8_t *counters;  // Counter tiles (x | y<<4), world order, 64 bytes
  const uint32_t *probe;    // dup mode: per cell, its first eight set-table probe slots (pyset_first)
};

template <bool LDS>
__device__ __forceinline__ Tables stage_tables(const void *__restrict__ tables, int n16, int quot_bytes) {
  Tables tb;
  if constexpr (LDS) {
    extern __shared__ uint4 oc_lds[];
    const uint4 *src = (const uint4 *)tables;
    // four named registers, not an array: a conditionally written array went to scratch
    const int i0 = threadIdx.x, i1 = i0 + blockDim.x, i2 = i1 + blockDim.x, i3 = i2 + blockDim.x;
    uint4 t0 = make_uint4(0, 0, 0, 0), t1 = t0, t2 = t0, t3 = t0;
    if (i0 < n16) t0 = src[i0];
    if (i1 < n16) t1 = src[i1];
    if (i2 < n16) t2 = src[i2];
    if (i3 < n16) t3 = src[i3];
    for (int idx = threadIdx.x + 4 * blockDim.x; idx < n16; idx += blockDim.x) oc_lds[idx] = src[idx];
    if (i0 < n16) oc_lds[i0] = t0;
    if (i1 < n16) oc_lds[i1] = t1;
    if (i2 < n16) oc_lds[i2] = t2;
    if (i3 < n16) oc_lds[i3] = t3;
    __syncthreads();
    tb.dist = (const uint8_t *)oc_lds + quot_bytes;
    tb.counters = (const uint8_t *)oc_lds + (n16 * 16 - OC_MAX_COUNTERS);
    tb.probe = (const uint32_t *)((const uint8_t *)oc_lds + (n16 * 16 - OC_MAX_COUNTERS - 4 * OC_MAX_CELLS));
  } else {
    tb.dist = (const uint8_t *)tables;   // quot_bytes is 0 since the quotient table went (v12)
    tb.counters = (const uint8_t *)tables + (n16 * 16 - OC_MAX_COUNTERS);
    tb.probe = (const uint32_t *)((const uint8_t *)tables + (n16 * 16 - OC_MAX_COUNTERS - 4 * OC_MAX_CELLS));
  }
  return tb;
}

// The map a wave's envs live on -- header, run configuration, table image -- as REFERENCES, so that each
// word is fetched where the code first needs it.  The launch's own (the by-value kernel argument:
// k_multi_step, k_obs, k_reset) or, in a map set, the record of the workgroup's map (k_mapset_*).
struct MapRef {
  const LevelHdr &L;
  const RunCfg &R;
  const void *const &tables;
  const int32_t &n16;
};
// Where a step finds its MapRef.  ref(): valid anywhere; ref_behind_loads(): called once, where the
// step has issued its state and action loads -- a map set looks its group's record up there and not
// before, so that those loads never wait for it.  LaunchMap: the launch's own map, the same references
// at both places.
struct LaunchMap {
  MapRef mp;
  __device__ __forceinline__ MapRef ref() const { return mp; }
  __device__ __forceinline__ MapRef ref_behind_loads() const { return mp; }
};

// Start cells of the items for a fresh episode of a random-* level
// (overcooked_environment.py:157-173: for every scattered letter, random.choice over ALL
// Counter tiles until one not yet taken by this phase comes up).  Either read from the
// caller's `placement` tensor ([M][n], x | y<<4; parity mode: the reference's own draws)
// or drawn here from the env's own PCG32 stream (`rng`, uint32 [n]; production mode --
// same distribution, not CPython's Mersenne Twister sequence).
__device__ __forceinline__ uint32_t pcg32(uint32_t &state) {
  state = state * 747796405u + 2891336453u;
  const uint32_t w = ((state >> ((state >> 28u) + 4u)) ^ state) * 277803737u;
  return (w >> 22u) ^ w;
}

template <int A, int M, int WS>
__device__ __forceinline__ void place_items_from(const Hdr &L, const Tables &tb, const int32_t *placement,
                                                 bool use_rng, uint32_t &st, int64_t n, int64_t i,
                                                 int32_t (&w)[WS]) {
  if (L.nscatter() == 0) return;  // uniform (compile-time in specialised builds)
  int pos[M];
#pragma unroll
  for (int k = 0; k < M; k++) pos[k] = w[A + k] & 255;
  if (use_rng) {
    unsigned long long taken = 0;
    for (int k = 0; k < (int)L.nscatter(); k++) {
      int idx = 0;
      bool ok = false;
      for (int attempt = 0; attempt < 64 && !ok; attempt++) {
        idx = (int)__umulhi(pcg32(st), L.ncounters());
        ok = !((taken >> idx) & 1);
      }
      for (int c = 0; c < (int)L.ncounters() && !ok; c++) {  // practically unreachable
        idx = c;
        ok = !((taken >> idx) & 1);
      }
      taken |= 1ull << idx;
      const int cell = tb.counters[idx];
      const int item = (int)L.scatter_item(k & 3);
#pragma unroll
      for (int m = 0; m < M; m++) pos[m] = (item == m) ? cell : pos[m];
    }
  } else if (placement != nullptr) {
#pragma unroll
    for (int k = 0; k < M; k++) pos[k] = placement[(int64_t)k * n + i] & 255;
  }
#pragma unroll
  for (int k = 0; k < M; k++) w[A + k] = (w[A + k] & ~255) | pos[k];
}

// read-modify-write form: the env's PCG32 state lives in rng[i]
template <int A, int M, int WS>
__device__ __forceinline__ void place_items(const Hdr &L, const Tables &tb, const int32_t *placement,
                                            uint32_t *rng, int64_t n, int64_t i, int32_t (&w)[WS]) {
  if (L.nscatter() == 0) return;
  const bool use_rng = rng != nullptr;
  uint32_t st = use_rng ? rng[i] : 0u;
  place_items_from<A, M, WS>(L, tb, placement, use_rng, st, n, i, w);
  if (use_rng) rng[i] = st;
}

struct StepArgs {
  LevelHdr L;
  RunCfg R;
  const void *tables;
  int32_t n16, quot_bytes;
  int32_t *state;
  const int32_t *actions;
  int32_t *reward;
  int32_t *done;
  double *shaping;
  int64_t *metrics;
  const int32_t *placement;
  uint32_t *rng;
  int64_t n;
  int32_t auto_reset;
  unsigned long long *timeline;   // OC_TIMELINE builds: this launch's record (else NULL, never read)
  int64_t timeline_stride;
};

// (leading scalars: preloaded kernel arguments, see k_multi_step)
// DUTY (see multi_step_body below): DUTY_STATE = reward, done, the state rows, metrics;
// DUTY_SHAPE = the reward shaping of sim agents 0 and 1.  Both = the whole step in one wave.
template <int A, int M, bool LDS, bool WT, bool DUP, bool PLAY, int DUTY, bool SPLIT>
__device__ __forceinline__ void step_body(int32_t *const state_, const int32_t *const actions_,
                                          int64_t *const metrics_, const int64_t n_, const int32_t launch_,
                                          const int32_t T_, const void *const tables_,
                                          const double inv_max_path_, const StepArgs &p) {
  constexpr bool D_STATE = (DUTY & 1) != 0, D_SHAPE = (DUTY & 2) != 0;
  using Out = RowsT<WT ? AUX_WT : 0>;
  OC_HDR_LOAD(p);
  const int block_ = launch_ & 0xFFFF;
  const bool auto_reset_ = (launch_ >> 16) & 1;
  // n < 2^31 / (4 * rows): fits_buffer().  Split: one workgroup = two waves over the same 64 envs.
  const int i = SPLIT ? (int)blockIdx.x * 64 + (int)(threadIdx.x & 63) : (int)blockIdx.x * block_ + (int)threadIdx.x;
  const bool valid = i < (int)n_;
  Tables tb;   // (global variant: formed after the state loads are issued, see k_multi_step)
  if constexpr (LDS) tb = stage_tables<true>(p.tables, p.n16, p.quot_bytes);
  MetricsSlot slot(metrics_, i);
  int reward = 0, done = 0, success = 0, comp = 0;
  bool err = false;
  if (valid) {
    constexpr int WS = state_words<A, M, DUP>();
    const Out st(state_, n_, WS, i);
    const Rows ac(actions_, n_, A, i);
    int32_t w[WS];
#pragma unroll
    for (int r = 0; r < WS; r++) w[r] = st.ld(r);
    int act[A];
#pragma unroll
    for (int a = 0; a < A; a++) act[a] = ac.ld(a);
    if constexpr (!LDS) tb = stage_tables<false>(tables_, p.n16, p.quot_bytes);
    Env<A, M, DUP> e;
    unpack<A, M, DUP>(e, w);
    // split: no state row is stored before both waves hold their copy of the state
    if constexpr (SPLIT) {
      asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      __builtin_amdgcn_s_waitcnt(WAIT_VMCNT0);   // (every load is back: see multi_step_body)
    }
    const int err_before = e.err;
    P done_p = 0;
    constexpr int B = A < 2 ? A : 2;
    ShapeIn<B> sin;
    ShapeLoads<B> sld;
#ifdef OC_STAMPS
    unsigned long long oc_tt[16];
#endif
    RunCfg R = p.R;
    R.T = T_;   // the preloaded copy
    env_step<A, M, DUP, PLAY ? 1 : 0, SPLIT>(L, R, tb.dist, tb.probe, e, act, reward, done, done_p, success, sin, sld OC_STAMP_PASS);
    comp = e.completed;
    err = e.err != err_before;
    ShapeQ<B> sq;
    if constexpr (D_SHAPE) shaping_lookup<B>(L, inv_max_path_, sin, sld, sq OC_STAMP_PASS);
    if constexpr (D_STATE) {
      Out(p.reward, p.n, 1, i).st(0, reward);
      Out(p.done, p.n, 1, i).st(0, done);
      if (L.nscatter() == 0) {   // uniform: a fixed level -- the fresh episode is a constant, selected word by word
        pack<A, M, DUP>(e, w);
        const P fresh = done_p & p_of(auto_reset_);
#pragma unroll
        for (int r = 0; r < WS; r++) w[r] = sel(fresh, L.init_words(r), w[r]);
      } else if (done && auto_reset_) {
#pragma unroll
        for (int r = 0; r < WS; r++) w[r] = L.init_words(r);
        place_items<A, M, WS>(L, tb, p.placement, p.rng, p.n, i, w);
      } else {
        pack<A, M, DUP>(e, w);
      }
#pragma unroll
      for (int r = 0; r < WS; r++) st.st(r, w[r]);
    }
    if constexpr (D_SHAPE) {
      double s0, s1;
      shaping_sum<B>(L, sin, sq, s0, s1 OC_STAMP_PASS);
      const Out sh(p.shaping, p.n, 2, i, 8);
      sh.st_f64(0, s0);
      sh.st_f64(1, s1);
    }
  }
  if constexpr (D_STATE) slot.add(metrics_ != nullptr, valid, done, success, reward, comp, err);
}

// OvercookedEnvironment.step for n envs.  SP = waves per 64 envs: 1, or 2 = split launch (128
// threads per workgroup: one wave steps and stores the state, the other computes the reward
// shaping -- the same idea as k_multi_step's four-way split, see multi_step_body).
template <int A, int M, bool LDS, bool WT, bool DUP, bool PLAY, int SP>
__global__ void __launch_bounds__(256) k_step(int32_t *const state_, const int32_t *const actions_,
                                              int64_t *const metrics_, const int64_t n_, const int32_t launch_,
                                              const int32_t T_, const void *const tables_,
                                              const double inv_max_path_, const StepArgs p) {
  // (tables_ / inv_max_path_ / T_ and, packed into launch_ = block | auto_reset << 16, the
  // auto-reset flag too: this kernel runs at the SGPR limit with 3-4 agents, and the compiler
  // otherwise loads each of them right before its first use and waits on the spot)
  static_assert(SP == 1 || (SP == 2 && !LDS), "waves per 64 envs");
  OC_TL_BEGIN();
  if constexpr (SP == 1) {
    step_body<A, M, LDS, WT, DUP, PLAY, 3, false>(state_, actions_, metrics_, n_, launch_, T_, tables_, inv_max_path_, p);
  } else {
    // (only launched by the specialised libraries, see oc_step)
    if (__builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6) == 0)
      step_body<A, M, LDS, WT, DUP, PLAY, 1, true>(state_, actions_, metrics_, n_, launch_, T_, tables_, inv_max_path_, p);
    else
      step_body<A, M, LDS, WT, DUP, PLAY, 2, true>(state_, actions_, metrics_, n_, launch_, T_, tables_, inv_max_path_, p);
  }
  OC_TL_END(p.timeline, p.timeline_stride, 1);
}

struct ObsArgs {
  LevelHdr L;
  RunCfg R;
  const int32_t *state;
  const int32_t *comm;
  void *obs;          // int32, int8 or float32 rows (cfg.obs_int8)
  double *timestep;
  int64_t n;
  oc_obs_cfg cfg;
};

// both viewers' rows of env i; `p`: the launch's tensors and configuration (ObsArgs, or a map set's SetObsArgs)
template <int A, int M, int OT, bool WT, bool DUP, typename ARGS>
__device__ __forceinline__ void obs_body(const LevelHdr &Lk, const RunCfg &R, const ARGS &p) {
  using Out = RowsT<WT ? AUX_WT : 0>;
  const Hdr L {Lk};
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  constexpr int WS = state_words<A, M, DUP>();
  const Rows st(p.state, p.n, WS, i);
  int32_t w[WS];
#pragma unroll
  for (int r = 0; r < WS; r++) w[r] = st.ld(r);
  Env<A, M, DUP> e;
  unpack<A, M, DUP>(e, w);
  const int C = p.cfg.num_comm;
  const int F = 22 + L.S() + 2 * C;
  const int c0 = p.comm[i], c1 = p.comm[p.n + i];
  const bool ego_blind = p.cfg.blind_mask & 1;
  const Out ob(p.obs, p.n, 2 * F, i, OT == 1 ? 1 : 4);
  const ObsSlots slots(R, false);
#pragma unroll
  for (int v = 0; v < 2; v++)
    env_obs<A, M, DUP, OT>(L, R, slots, e, v, p.cfg.fow_radius, (p.cfg.blind_mask >> v) & 1, ego_blind, C, c0, c1, ob, v * F);
  Out(p.timestep, p.n, 1, i, 8).st_f64(0, timestep_of(e.t, R));  // overcooked_env.py:146
}

template <int A, int M, int OT, bool WT, bool DUP>
__global__ void __launch_bounds__(256) k_obs(const ObsArgs p) {
  obs_body<A, M, OT, WT, DUP>(p.L, p.R, p);
}

struct ImageArgs {
  LevelHdr L;
  const int32_t *state;
  int32_t *out;       // [2][7][ceil(W*H / 4)][n]: four consecutive cells of a plane per dword
  int8_t *holding;    // [2][n]
  int64_t n;
  int32_t radius;
};

// OvercookedMultiEnv.get_partial_observability_FOW for both viewers
// (gym_comm/envs/overcooked_env.py:161-202; the image-style observation the reference
// defines but does not call).  Plane k of viewer v at cell (x, y) -- the reference's
// map[k][x][y] -- is byte (x*H + y) of the plane: plane 0 the tile type, planes 1.. "agent i
// stands here" (:183-185 -- with 3+ agents these overwrite the content planes, as in the
// reference), planes 3 + channel the contents (Food: state_index + 1, Plate: 1); cells farther
// than `radius` (manhattan) from the viewer are -1 in every plane.  A lane packs FOUR consecutive
// cells of a plane of its env into one dword (little-endian, zero padded past the last cell), so
// a wave stores 256 contiguous bytes per instruction.
// Work per env is organised by QUAD, not by byte: the fog bytes of a quad are formed once per
// viewer and reused by its seven planes; an agent / item contributes to the one quad its cell
// falls into (a compare and a select per quad); a plane's dword is then one bit-field insert
// (fog bytes win) and one store.  ~1 100 VALU + 182 stores per wave at 7x7 -- the first version
// walked the 343 bytes of a viewer one by one, ~120 instructions each (56 us per launch at 4 096
// envs; this one: see DESIGN.md).
template <int A, int M, bool DUP>
__global__ void __launch_bounds__(256) k_obs_image(const ImageArgs p) {
  OC_HDR_LOAD(p);
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  constexpr int WS = state_words<A, M, DUP>();
  const Rows st(p.state, p.n, WS, i);
  int32_t w[WS];
#pragma unroll
  for (int r = 0; r < WS; r++) w[r] = st.ld(r);
  Env<A, M, DUP> e;
  unpack<A, M, DUP>(e, w);
  const int W = L.W(), H = L.H();
  const int ncell = W * H, Q = (ncell + 3) >> 2;
  const __amdgpu_buffer_rsrc_t rsrc =
      __builtin_amdgcn_make_buffer_rsrc(p.out, 0, (int)(2 * 7 * Q * p.n * 4), 0x00020000);
  // per agent / item: the quad its cell (x-major index x*H + y) falls into and its byte there
  int aq[A], abyte[A];
#pragma unroll
  for (int a = 0; a < A; a++) {
    const int c = (int)__umul24((unsigned)px(e.ap[a]), (unsigned)H) + py(e.ap[a]);
    aq[a] = c >> 2;
    abyte[a] = 8 * (c & 3);
  }
  int iq[M], ishift[M], ival[M];
#pragma unroll
  for (int m = 0; m < M; m++) {
    const int pos = ipos(e.iw[m]);
    const int c = (int)__umul24((unsigned)px(pos), (unsigned)H) + py(pos);
    iq[m] = c >> 2;
    ishift[m] = 8 * (c & 3);
    ival[m] = item_type(L, m) == OC_PLATE ? 1 : ichop(e.iw[m]) + 1;
    // the last writer in world order wins (:171-178): an item gives way to a later one of its
    // type on the same cell (only in levels that repeat a type)
    bool later = false;
#pragma unroll
    for (int o = 0; o < M; o++)
      if (o != m && item_type(L, o) == item_type(L, m))   // uniform
        later |= ipos(e.iw[o]) == pos && (e.iw[o] & IW_SEQ) > (e.iw[m] & IW_SEQ);
    iq[m] = later ? -1 : iq[m];
  }
  const int vx[2] = {px(e.ap[0]), px(e.ap[1])}, vy[2] = {py(e.ap[0]), py(e.ap[1])};
  int x = 0, y = 0;   // cell of the quad's first byte, advanced incrementally (uniform)
  for (int q = 0; q < Q; q++) {
    unsigned fog[2] = {0u, 0u}, tile = 0u;
#pragma unroll
    for (int b = 0; b < 4; b++)
      if (4 * q + b < ncell) {   // uniform
        tile |= (unsigned)cell_type(L, y * W + x) << (8 * b);   // uniform: SALU
#pragma unroll
        for (int v = 0; v < 2; v++)
          fog[v] |= (int)sad_u32((unsigned)x, (unsigned)vx[v], sad_u32((unsigned)y, (unsigned)vy[v], 0u)) > p.radius
                        ? 0xFFu << (8 * b) : 0u;
        if (++y == H) y = 0, x++;
      }
#pragma unroll
    for (int k = 0; k < 7; k++) {
      unsigned val = k == 0 ? tile : 0u;
      if (k >= 3) {
#pragma unroll
        for (int m = 0; m < M; m++)
          if (item_type(L, m) + 3 == k)   // uniform
            val |= iq[m] == q ? (unsigned)ival[m] << ishift[m] : 0u;
      }
      if (k >= 1 && k <= A) {   // agent k-1 stands here: 1, over whatever the plane held at that cell
        const int a = k - 1;
        val = aq[a] == q ? (val & ~(0xFFu << abyte[a])) | (1u << abyte[a]) : val;
      }
#pragma unroll
      for (int v = 0; v < 2; v++)
        __builtin_amdgcn_raw_buffer_store_b32((int)(val | fog[v]), rsrc, (int)i * 4,
                                              (int)(((v * 7 + k) * Q + q) * p.n * 4), AUX_WT);
    }
  }
  p.holding[i] = e.ahp[0] != 0;
  p.holding[p.n + i] = e.ahp[1] != 0;
}

struct ResetArgs {
  LevelHdr L;
  const void *tables;
  int32_t n16, quot_bytes;
  int32_t *state;
  const int32_t *mask;
  const int32_t *placement;
  uint32_t *rng;
  int64_t n;
};

// OvercookedEnvironment.reset() (overcooked_environment.py:180-206), masked; `p`: the launch's tensors
// (ResetArgs, or a map set's SetResetArgs)
template <int A, int M, bool DUP, typename ARGS>
__device__ __forceinline__ void reset_body(const LevelHdr &Lk, const void *const &tables, const int32_t &n16,
                                           const ARGS &p) {
  const Hdr L {Lk};
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.n) return;
  if (p.mask != nullptr && p.mask[i] == 0) return;
  constexpr int WS = state_words<A, M, DUP>();
  const Tables tb = stage_tables<false>(tables, n16, 0);
  int32_t w[WS];
#pragma unroll
  for (int r = 0; r < WS; r++) w[r] = L.init_words(r);
  place_items<A, M, WS>(L, tb, p.placement, p.rng, p.n, i, w);
#pragma unroll
  for (int r = 0; r < WS; r++) p.state[(int64_t)r * p.n + i] = w[r];
}

template <int A, int M, bool DUP>
__global__ void __launch_bounds__(256) k_reset(const ResetArgs p) {
  reset_body<A, M, DUP>(p.L, p.tables, p.n16, p);
}

// Uniform random (move, comm) indices of one player (include/oc_hip.h: oc_random_actions)
__global__ void __launch_bounds__(256) k_random_actions(uint32_t *rng, int32_t *move_row, int32_t *comm_row,
                                                        uint32_t num_comm, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t st = rng[i];
  move_row[i] = (int32_t)__umulhi(pcg32(st), 4u);
  comm_row[i] = (int32_t)__umulhi(pcg32(st), num_comm);
  rng[i] = st;
}

struct MultiArgs {
  LevelHdr L;
  RunCfg R;
  const void *tables;
  int32_t n16, quot_bytes;
  int32_t *state;
  int32_t *comm;
  const int32_t *actions;
  void *obs;          // int32, int8 or float32 rows (cfg.obs.obs_int8)
  double *timestep;
  double *reward;
  int32_t *done;
  int32_t *sparse;
  int64_t *metrics;
  const int32_t *placement;
  uint32_t *rng;
  oc_step_opts opt;      // optional inputs / outputs (include/oc_hip.h), all NULL = off
  int64_t n;
  int32_t auto_reset;
  oc_wrap_cfg cfg;
  oc_step_policy pol[2]; // opt.policy by value (it is a host pointer), used by the POL variants
  int32_t pol_ksteps;
  unsigned long long *timeline;   // OC_TIMELINE builds: this launch's record (else NULL, never read)
  int64_t timeline_stride;
};

// OvercookedMultiEnv.multi_step (gym_comm/envs/overcooked_env.py:207-282), 2 agents.
// XO = 0: the plain step in the wrapper's standard configuration -- actions from the four
// rows, no episode statistics (`p.opt` is not even looked at), communication on, not ego-led,
// both players CAN_MOVE, ego = sim agent 0, nobody BLIND, arglist.play off (the reference's
// env_args*.json and BASELINE.md section 3) -- with those settings folded: no selects on them, no
// BLIND branch and none of the register copies its join costs.
// XO = 1: the same standard configuration, still folded, plus oc_step_opts' action sources
// ([n][2] pairs, the in-kernel partner), episode statistics and the fused policies: what
// OvercookedVecEnv launches with the reference's own run configurations (round 3: until then
// every option landed in ONE general variant and step_tensors paid for run-time `play` and
// wrapper-configuration selects it never uses -- specialised libraries only).
// XO = 2: the general variant -- any wrapper configuration, arglist.play at run time, and the options.
//
// DUTY: which of the step's OUTPUTS this wave produces.  Everything up to done/reward is needed by
// every output and is computed by every wave; what follows splits four ways:
//   DUTY_STATE  comm rows, done, sparse reward, the state rows, the metrics counters (and the
//               in-place words of the optional random streams)
//   DUTY_SHAPE  the reward shaping (distance lookups, fp64 sums), the shaped reward, episode statistics
//   DUTY_OBS0 / DUTY_OBS1  get_observation2 for viewer 0 (+ the timestep) / viewer 1
// DUTY_ALL is the whole step in one wave.  A *split* launch (k_multi_step<..., SP = 4>: four waves
// per 64 envs in one workgroup, i.e. one wave on each SIMD of a CU) gives each wave one duty.  Why:
// at the BASELINE batch sizes a step puts ONE wave on 64 ... 256 of the chip's 1 024 SIMDs, a lone
// wave issues an instruction every ~7 cycles whatever the other SIMDs do, and the step lasts as
// long as that wave's instruction stream (~950 instructions).  The stream is therefore cut where
// the data flow forks, and the three idle SIMDs next door run the branches side by side: ~620
// instructions per wave instead of ~950 (the part before the fork is recomputed by every wave --
// free while the batch leaves SIMDs idle; each arm is compiled on its own, so the loads and the
// arithmetic only another duty needs are gone from it).  The state is updated in place, so a split
// workgroup passes one s_barrier between "every wave holds its copy of the state" and the first
// store of anything a later-starting wave might still have to read.
// Measured (tools/split_sweep.sh, MI355X): tomato-2, 4 096 envs 3.55 -> 3.07 us per step; equal at
// 32 768 envs (every SIMD has a wave of its own by then), slower beyond: split_for().
constexpr int DUTY_STATE = 1, DUTY_SHAPE = 2, DUTY_OBS0 = 4, DUTY_OBS1 = 8, DUTY_ALL = 15;

// Split launch with the policies fused: both viewers' observation rows of the workgroup's 64 envs
// as floats, [viewer][row][env], and the timestep -- written by the observation waves, read by all
// four waves' policy passes behind the second barrier.  (Function templates of their own: ONE LDS
// array for the four arms of the kernel, which are four instantiations of multi_step_body.)
template <int ROWS>
__device__ __forceinline__ float *pol_lds_feat() {
  __shared__ float a[2 * ROWS * 64];
  return a;
}
__device__ __forceinline__ float *pol_lds_ts() {
  __shared__ float t[64];
  return t;
}

// POL (general variant only): the closed loop in one launch -- behind the step, the wave(s) evaluate
// both players' MLP policies (oc_policy_device.h) on the observation rows just written and put the
// NEXT step's (move, comm) pairs where this step read its own (oc_step_opts.policy).  One pass =
// one wave x 32 envs; a split workgroup gives each of its four waves one (viewer, half) pass
// behind a second barrier ("every observation row of these 64 envs is written"), a lone wave
// runs all four.
// LN (lane-split launch, see LaneParts): lanes per env, 1 or 2.  A workgroup of LN > 1 is still
// four duty waves and one barrier but covers 64 / LN envs; every lane runs its env's step up to
// done/reward (the parts of an env compute identical values), an observation wave's parts then
// store different rows, and the state and shaping waves work in part 0 alone.
template <int M, bool LDS, int OT, bool WT, bool DUP, int XO, int DUTY, bool SPLIT, bool POL = false, int LN = 1,
          typename ARGS = MultiArgs, typename MAPS = LaunchMap>
__device__ __forceinline__ void multi_step_body(int32_t *const state_, const int32_t *const actions_,
                                                int32_t *const comm_, int64_t *const metrics_,
                                                const int32_t n_, const int32_t block_, const void *const ego_src_,
                                                const void *const alt_src_, const ARGS &p, const MAPS &maps) {
  constexpr int A = 2;
  constexpr bool D_STATE = (DUTY & DUTY_STATE) != 0, D_SHAPE = (DUTY & DUTY_SHAPE) != 0;
  using Out = RowsT<WT ? AUX_WT : 0>;
#ifdef OC_SPECIALIZED
  constexpr int POL_ROWS = (POL && SPLIT) ? 22 + OC_SPEC_HDR.S + 8 : 1;   // F at most: 4 comm channels
#else
  constexpr int POL_ROWS = 1;
#endif
  // n < 2^31 / (4 * rows): fits_buffer().  Split: one workgroup = SP waves over the same 64 envs.
  static_assert(LN == 1 || (SPLIT && XO == 0 && !POL && !LDS && DUTY != DUTY_ALL), "lane-split: the plain four-way split only");
  constexpr int EPW = 64 / LN;   // envs per split workgroup
  const int i = SPLIT ? (int)blockIdx.x * EPW + (int)(threadIdx.x & (EPW - 1))
                      : (int)blockIdx.x * (block_ & 0xFFFF) + (int)threadIdx.x;
  // (lane-split: only the observation waves have work for the parts behind part 0)
  constexpr bool PART0_ONLY = LN > 1 && (DUTY & (DUTY_OBS0 | DUTY_OBS1)) == 0;
  const bool valid = PART0_ONLY ? (i < (int)n_ && (int)(threadIdx.x & 63) < EPW) : i < (int)n_;
  const bool ego_from_pairs = XO != 0 && ((block_ >> 16) & 1), alt_from_pairs = XO != 0 && ((block_ >> 17) & 1),
             alt_from_rng = XO != 0 && ((block_ >> 18) & 1), pairs64 = XO != 0 && ((block_ >> 19) & 1);
#ifdef OC_STAMPS
  unsigned long long oc_tt[16];
  for (int k = 0; k < 16; k++) oc_tt[k] = 0;
#endif
  OC_STAMP(0);
  // LDS variant: staged first (its loads overlap the state loads).  Global variant: the table
  // base pointers are formed AFTER the state loads are issued -- formed first, their scalar
  // kernarg load was waited for before a single vector load had left.
  Tables tb;
  if constexpr (LDS) tb = stage_tables<true>(maps.ref().tables, maps.ref().n16, p.quot_bytes);
  MetricsSlot slot(metrics_, i);
  int reward = 0, done = 0, success = 0, comp = 0;
  bool err = false;
  // (POL, split: which (viewer, half) pass this wave runs behind the step -- viewer 0 / first half
  // on the OBS0 wave, viewer 1 / first half on OBS1, the second halves on the STATE and SHAPE waves)
  constexpr int POL_MINE = (DUTY == DUTY_OBS0) ? 0 : (DUTY == DUTY_OBS1) ? 2 : (DUTY == DUTY_STATE) ? 1 : 3;
  constexpr int POL_VIEWER = POL_MINE >> 1;
  [[maybe_unused]] ocpol::Weights pol_w;
  if constexpr (POL && SPLIT) {
    // This wave's pass is for viewer POL_VIEWER: its share of that player's weights is fetched
    // now, under the wait for the state -- by EVERY lane: a lane's fragments are rows of the weight
    // matrices, needed whether or not the lane has an env of its own.
    ocpol::load_weights(pol_w, p.pol[POL_VIEWER].w1, p.pol[POL_VIEWER].w2, p.pol[POL_VIEWER].b2,
                        (int)threadIdx.x & 63, p.pol_ksteps);
  }
  if (valid) {
    // (Tried: the state loads ahead of this tail-lane test -- v_cmp -> s_and_saveexec costs ~16 cycles
    // in front of the first load.  Nothing at 4 096 envs, and salad-2 x 32 768, two waves per SIMD,
    // went from 3.96 to 4.34 us: the shaping wave of a workgroup ended 0.2 us later.  Left as it was.)
    constexpr int WS = state_words<A, M, DUP>();
    const Out st(state_, n_, WS, i), cm(comm_, n_, 2, i);
    int32_t w[WS];
#pragma unroll
    for (int r = 0; r < WS; r++) w[r] = st.ld(r);
    // The two players' (move, comm): rows 0..3 of `actions` [4][n] -- or, per player, an
    // [n][2] array of pairs (the batched form of multi_step's ego_action / alt_action tuples: a
    // policy's [n, 2] output is consumed as it lies); the partner may also be drawn here,
    // uniformly from the env's own PCG32 stream (oc_step_opts).  All three tests are uniform.
    // ISSUE PHASE: every load of the step goes out before any loaded word is touched.  (Until
    // round 3 each source decoded its words inside its own branch -- the int64 range check, the
    // PCG32 draw -- which put an s_waitcnt vmcnt(0) for ALL loads issued so far, the state's
    // included, in front of the loads still to come: the episode statistics' three loads started
    // a second memory round trip.  ego pairs + in-kernel partner + statistics: 3.91 us per step at
    // 4 096 envs against 2.9 plain.)
    typedef int v2i __attribute__((ext_vector_type(2)));
    typedef int v4i __attribute__((ext_vector_type(4)));
    // raw words as they are loaded (no shuffling here: a move of a loaded word is a wait for it):
    // int64 pairs {move lo, move hi, comm lo, comm hi}; int32 pairs and rows {move, comm}.
    // XO != 0: NO BRANCH over the sources.  Per player ONE 16-byte load serves both [n][2] forms --
    // int64 pairs (lane offset 16 i: the pair), int32 pairs (8 i: the pair and the next env's) -- two
    // dword loads serve the rows and one the partner's PCG32 word, each through a buffer descriptor
    // whose length is 0 when the form is not in use: a load past the end of its buffer returns 0 and
    // touches no memory.  (A chain of uniform branches, one
    // load per arm, is laid out as consecutive `if`s with flag words and a value merged at every
    // join; the wait-count pass follows EVERY path through them, found a register written on one path
    // -- a zero default, a copy for the merge, an address formed in a destination register -- with a
    // load outstanding on another, and put an s_waitcnt vmcnt(0) into the common path in front of the
    // episode statistics' loads: a second memory round trip for int32 pairs + statistics and for the
    // fused policies.)
    v4i eq = {0, 0, 0, 0}, aq = {0, 0, 0, 0};
    v2i er = {0, 0}, ar = {0, 0};
    uint32_t alt_rs = 0;
    if constexpr (XO != 0) {
      const auto desc = [&](const void *base, bool on, int bytes) {
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<void *>(base), 0, on ? bytes : 0, 0x00020000);
      };
      const int sh = pairs64 ? 4 : 3;
      const __amdgpu_buffer_rsrc_t d_er = desc(actions_, !ego_from_pairs, (int)n_ * 16),
                                   d_ar = desc(actions_, !alt_from_pairs && !alt_from_rng, (int)n_ * 16),
                                   d_eq = desc(ego_src_, ego_from_pairs, (int)n_ << sh),
                                   d_aq = desc(alt_src_, alt_from_pairs && !alt_from_rng, (int)n_ << sh),
                                   d_rs = desc(alt_src_, alt_from_rng, (int)n_ * 4);
      const int off4 = i << 2, offq = i << sh, row = (int)n_ * 4;
      eq = (v4i)__builtin_amdgcn_raw_buffer_load_b128(d_eq, offq, 0, 0);
      aq = (v4i)__builtin_amdgcn_raw_buffer_load_b128(d_aq, offq, 0, 0);
      alt_rs = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(d_rs, off4, 0, 0);
      er.x = __builtin_amdgcn_raw_buffer_load_b32(d_er, off4, 0, 0);
      er.y = __builtin_amdgcn_raw_buffer_load_b32(d_er, off4, row, 0);
      ar.x = __builtin_amdgcn_raw_buffer_load_b32(d_ar, off4, 2 * row, 0);
      ar.y = __builtin_amdgcn_raw_buffer_load_b32(d_ar, off4, 3 * row, 0);
    } else {
      const Rows ac(actions_, n_, 4, i);
      er.x = ac.ld(0), er.y = ac.ld(1);
      ar.x = ac.ld(2), ar.y = ac.ld(3);
    }
    // the env's map: the launch's, or (map sets) the group's record, looked up only now
    const MapRef mp = maps.ref_behind_loads();
    const Hdr L {mp.L};
    if constexpr (!LDS) tb = stage_tables<false>(mp.tables, mp.n16, 0);   // (quot_bytes: 0 since v12, and unread here)
    // the output pointers are needed hundreds of instructions from here, where the compiler
    // would place their scalar loads -- and a wait on them -- in the middle of the step; fetch
    // them now, under the wait for the state that has to be served anyway
    asm volatile("" ::"s"(tb.dist), "s"(p.obs), "s"(p.timestep), "s"(p.reward), "s"(p.done),
                 "s"(p.sparse), "s"(p.auto_reset), "s"(mp.R.inv_T), "s"(mp.R.inv_max_path));
    if constexpr (XO != 0) asm volatile("" ::"s"(p.opt.ep_return), "s"(p.opt.ep_length));
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
    // structure library: the map's geometry is a kernel argument; the first things the step
    // needs of it -- row length, tile planes, the Delivery tile -- are fetched here as well
    asm volatile("" ::"s"(L.W()), "s"(L.ncells()), "s"(L.max_path()), "s"(L.cell_lo(0)), "s"(L.cell_hi(0)),
                 "s"(L.deliv_pos(0)));
#endif
    // episode statistics: the running return / length and the previous step's done flag are
    // loaded now, with the state, and consumed after the last store of the step.  (Loading the
    // totals behind the barrier instead -- they are the shaping wave's own -- was slower: vmcnt
    // retires in order, so the shaping's distance lookups then waited for them: 3.64 -> 3.90 us.)
    double ep_ret = 0.0;
    int ep_len = 0, prev_done = 0;
    if (XO != 0 && p.opt.ep_return != nullptr) {   // uniform
      const Rows er(p.opt.ep_return, n_, 1, i, 8);
      ep_ret = __builtin_bit_cast(double, (v2i)__builtin_amdgcn_raw_buffer_load_b64(er.rsrc, er.voff, 0, 0));
      ep_len = Rows(p.opt.ep_length, n_, 1, i).ld(0);
      prev_done = Rows(p.done, n_, 1, i).ld(0);
    }
    Env<A, M, DUP> e;
    unpack<A, M, DUP>(e, w);
    // What the observation rows need of the LAUNCH alone -- the descriptor of the tensor, which
    // bit of `completed` each subtask row shows and, in a split workgroup's observation waves, the
    // byte offset of every row the wave will store -- is formed here, under the wait for the state:
    // the ~30 row stores are the tail of the step's longest waves, and every scalar instruction
    // among them costs a lone wave its ~4 cycles.
    const int C = p.cfg.obs.num_comm;
    const int F = 22 + L.S() + 2 * C;
    const Out ob(p.obs, p.n, 2 * F, i, OT == 1 ? 1 : 4);
    constexpr bool OBS_ONLY = SPLIT && (DUTY == DUTY_OBS0 || DUTY == DUTY_OBS1);
    // which observation arm of a split workgroup stores the timestep (-DOC_TS_OBS1: viewer 1's, a
    // measurement variant, profiles/step_prefix_ab.txt; with the policies fused always viewer 0's,
    // which hands it to the policy passes)
#ifdef OC_TS_OBS1
    constexpr int TS_DUTY = POL ? DUTY_OBS0 : DUTY_OBS1;
#else
    constexpr int TS_DUTY = DUTY_OBS0;
#endif
#ifdef OC_SPECIALIZED
    // (the plain variant only, and at most 40 offsets -- salad's 22 + 9 + 8 fit beside the step's own
    // ~64 SGPRs; the options variants and a level with more subtasks began to spill SGPRs to VGPR
    // lanes.  Rows past the table are stored as before, with a multiply.)
    constexpr int NPRE_ALL = 22 + (int)OC_SPEC_HDR.S + 8;   // up to four comm channels
    constexpr int NPRE = (OBS_ONLY && !POL && XO == 0) ? (NPRE_ALL < 40 ? NPRE_ALL : 40) : 0;
#else
    constexpr int NPRE = 0;   // (the number of subtask rows is a run-time value)
#endif
    const ObsSlots slots(mp.R, NPRE != 0);
    const RowsPreT<WT ? AUX_WT : 0, NPRE> obp(ob, DUTY == DUTY_OBS1 ? F : 0);
    if constexpr (NPRE != 0) asm volatile("" ::"s"(ob.rsrc));   // (the descriptor's words as well)
#ifdef OC_SPECIALIZED
    // (lane-split: what this lane's part adds to the offsets and selects, formed here as well)
    using Parts = std::conditional_t<(LN > 1 && OBS_ONLY), LaneParts<(LN > 1 ? LN : 2)>, NoParts>;
    [[maybe_unused]] const Parts parts(ob, slots, C);
#endif
    const Out tso(p.timestep, p.n, 1, i, 8);
    if constexpr (NPRE != 0 && DUTY == TS_DUTY) asm volatile("" ::"s"(tso.rsrc), "v"(tso.voff));
    // split: nothing that is updated in place -- state rows, the words of the random streams, the
    // done row the episode statistics read -- may be stored before every wave of the workgroup
    // holds its copy
    uint32_t place_rs = 0;
    if constexpr (SPLIT) {
      if (L.nscatter() != 0 && p.rng != nullptr) place_rs = (uint32_t)Rows(p.rng, n_, 1, i).ld(0);   // uniform
      // (the raw action words pass THROUGH this statement: the optimiser otherwise threads the decode
      // below back into the branch that issued each load, and its wait in front of the later loads)
      if constexpr (XO != 0)
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" : "+v"(eq), "+v"(aq), "+v"(er), "+v"(ar), "+v"(alt_rs)::"memory");
      else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
      // The statement above has waited for every load, but the compiler's wait-count pass does not
      // read asm text: it put an s_waitcnt vmcnt(N) in front of the first use of each loaded word in
      // the decode below, up to nine of them, an issue slot each.  One wait it does see tells it that
      // every load is back.
      // (Tried: the words as "+v" operands of an empty statement behind the barrier, newest load
      // first.  One wait in the observation arms, nine in the other two, where the scheduler issues
      // the action loads first -- and the comm words the shaping arm never reads stayed alive.)
      __builtin_amdgcn_s_waitcnt(WAIT_VMCNT0);
      // (the offsets pinned above hang on scalar loads, and this statement is ordered behind their
      // pins: left alone, the scheduler fills that latency with the step's arithmetic and the
      // barrier sinks ~400 instructions, to where the first store needs it)
      if constexpr (NPRE != 0) __builtin_amdgcn_sched_barrier(0);
    } else if constexpr (XO != 0) {
      asm volatile("" : "+v"(eq), "+v"(aq), "+v"(er), "+v"(ar), "+v"(alt_rs));
    }
    // DECODE PHASE (every load is out; a split workgroup is past its barrier: branches are free of
    // waits here).  A form not in use read 0; an int64 outside int32 is no valid index: -1.
    int ego_mv = er.x, ego_cm = er.y, alt_mv = ar.x, alt_cm = ar.y;
    if constexpr (XO != 0) {
      const auto narrow = [](int lo, int hi) { return lo | ~p_eq_any(hi, lo >> 31); };
      if (pairs64) {   // uniform
        ego_mv |= narrow(eq.x, eq.y), ego_cm |= narrow(eq.z, eq.w);
        alt_mv |= narrow(aq.x, aq.y), alt_cm |= narrow(aq.z, aq.w);
      } else {
        ego_mv |= eq.x, ego_cm |= eq.y;
        alt_mv |= aq.x, alt_cm |= aq.y;
      }
    }
    if (alt_from_rng) {   // uniform: the partner's draw, two steps of the env's PCG32 stream
      alt_mv = (int)__umulhi(pcg32(alt_rs), 4u);
      alt_cm = (int)__umulhi(pcg32(alt_rs), (uint32_t)p.cfg.obs.num_comm);
      if (!SPLIT || D_STATE) {   // (split: stored by the wave that owns the state, behind the barrier)
        Rows(alt_src_, n_, 1, i).st(0, (int)alt_rs);
        if (p.opt.alt_played != nullptr) {
          const Rows ap(p.opt.alt_played, n_, 2, i);
          ap.st(0, alt_mv);
          ap.st(1, alt_cm);
        }
      }
    }
    OC_STAMP(1);   // state + actions arrived
    // comm one-hots (:227-246); an index the reference's one_hot[idx] = 1 would raise on is
    // flagged (OC_ERR_ACTION) and sends nothing
    // (XO == 2: any wrapper configuration; 0 and 1 run the standard one, folded)
    const bool cfg_comm_on = XO == 2 ? p.cfg.communication_on != 0 : true, cfg_ego_led = XO == 2 ? p.cfg.ego_led != 0 : false;
    const int cfg_can_move = XO == 2 ? p.cfg.can_move_mask : 3, cfg_ego_idx = XO == 2 ? p.cfg.ego_agent_idx : 0;
    const int cfg_blind = XO == 2 ? p.cfg.obs.blind_mask : 0;
    const unsigned NC = (unsigned)p.cfg.obs.num_comm;
    // (per-lane predicates are P words, 0 / -1, see `hide`; the cfg_* tests are wave-uniform)
    const bool ego_talks = cfg_comm_on, alt_talks = cfg_comm_on && !cfg_ego_led;
    const P ego_cm_bad = p_geu_any((unsigned)ego_cm, NC), alt_cm_bad = p_geu_any((unsigned)alt_cm, NC);
    const P bad_cm = (p_of(ego_talks) & ego_cm_bad) | (p_of(alt_talks) & alt_cm_bad);
    const int c0 = ego_talks ? (ego_cm | ego_cm_bad) : -1;    // the index, or -1 = nothing sent
    const int c1 = alt_talks ? (alt_cm | alt_cm_bad) : -1;
    if constexpr (D_STATE) {
      cm.st(0, c0);
      cm.st(1, c1);
    }
    // NAV_ACTIONS lookup (both indices, moved or not: :248) + CAN_MOVE gating + ego_agent_idx
    // (:250-262); NAV_ACTIONS[idx] raises for idx > 3: flagged, executed as (0, 0)
    const P bad_mv = p_gtu_any((unsigned)ego_mv, 3u) | p_gtu_any((unsigned)alt_mv, 3u);
    const int em = (cfg_can_move & 1) ? (int)min((unsigned)ego_mv, 4u) : OC_ACT_NOOP;   // (> 3 -> 4 = OC_ACT_NOOP)
    const int am = (cfg_can_move & 2) ? (int)min((unsigned)alt_mv, 4u) : OC_ACT_NOOP;
    int act[A];
    act[0] = cfg_ego_idx == 0 ? em : am;
    act[1] = cfg_ego_idx == 0 ? am : em;
    const int err_before = e.err;
    P done_p = 0;
    e.err |= (bad_mv | bad_cm) & OC_ERR_ACTION;
    ShapeIn<2> sin;
    ShapeLoads<2> sld;
    // (the plain variant is only launched for play == 0; the general one reads the flag)
    env_step<A, M, DUP, XO == 2 ? 2 : 0, SPLIT>(L, mp.R, tb.dist, tb.probe, e, act, reward, done, done_p, success, sin, sld OC_STAMP_PASS);
    comp = e.completed;
    err = e.err != err_before;
    if constexpr (D_STATE) {
      Out(p.done, p.n, 1, i).st(0, done);
#ifndef OC_STAMPS
      if (p.sparse != nullptr) Out(p.sparse, p.n, 1, i).st(0, reward);
#endif
    }
    if constexpr (DUTY != DUTY_SHAPE) {   // (the shaping reads the pre-reset env only, through `sin`)
      if ((DUTY & (DUTY_OBS0 | DUTY_OBS1)) == 0 && L.nscatter() == 0) {
        // the state wave of a split launch, a fixed level (uniform; compile-time in specialised
        // builds): the fresh episode is a constant, selected word by word -- a branch on `done` is
        // v_cmp -> s_and_saveexec, a scalar read of a vector-written mask (see `hide`).  (A wave that
        // goes on to the observations keeps the branch: it would have to unpack the words again.)
        pack<A, M, DUP>(e, w);
        const P fresh = done_p & p_of(p.auto_reset != 0);
#pragma unroll
        for (int r = 0; r < WS; r++) w[r] = sel(fresh, L.init_words(r), w[r]);
      } else if (OBS_ONLY && L.nscatter() == 0) {
        // an observation wave of a split launch, a fixed level: the same select, on the fields
        // the observation reads (the rest is dead code here), instead of the branch
        int32_t w0[WS];
#pragma unroll
        for (int r = 0; r < WS; r++) w0[r] = L.init_words(r);
        Env<A, M, DUP> e0;
        unpack<A, M, DUP>(e0, w0);
        const P fresh = done_p & p_of(p.auto_reset != 0);
#pragma unroll
        for (int a = 0; a < A; a++) e.ap[a] = sel(fresh, e0.ap[a], e.ap[a]), e.ahp[a] = sel(fresh, e0.ahp[a], e.ahp[a]);
#pragma unroll
        for (int k = 0; k < M; k++) e.iw[k] = sel(fresh, e0.iw[k], e.iw[k]);
        e.t = sel(fresh, e0.t, e.t);
        e.completed = sel(fresh, e0.completed, e.completed);
      } else if (done && p.auto_reset) {
#pragma unroll
        for (int r = 0; r < WS; r++) w[r] = L.init_words(r);
        if constexpr (SPLIT) {   // every wave draws the same cells from its copy of the stream's word
          place_items_from<A, M, WS>(L, tb, p.placement, p.rng != nullptr, place_rs, p.n, i, w);
          if (D_STATE && L.nscatter() != 0 && p.rng != nullptr) p.rng[i] = place_rs;
        } else {
          place_items<A, M, WS>(L, tb, p.placement, p.rng, p.n, i, w);
        }
        unpack<A, M, DUP>(e, w);
      } else {
        pack<A, M, DUP>(e, w);
      }
    }
    if constexpr (D_STATE) {
#pragma unroll
      for (int r = 0; r < WS; r++) st.st(r, w[r]);
    }
    // The timestep: formed here, where `t` is final, and -- in a split workgroup's observation arm --
    // stored in front of the arm's rows, so that its fp64 chain runs under the observation's own
    // arithmetic.  (It used to follow the last row store of viewer 0's arm, the longest.)
    constexpr bool TS_MINE = OBS_ONLY ? DUTY == TS_DUTY : (DUTY & DUTY_OBS0) != 0;
    [[maybe_unused]] double tsd = 0.0;
    if constexpr (TS_MINE && OBS_ONLY && !POL) tsd = timestep_of(e.t, mp.R);
    if constexpr (TS_MINE && OBS_ONLY && !POL) tso.st_f64(0, tsd);
    ShapeQ<2> sq;
    if constexpr (D_SHAPE) shaping_lookup<2>(L, mp.R.inv_max_path, sin, sld, sq OC_STAMP_PASS);
    const bool ego_blind = cfg_blind & 1;
    if constexpr (POL && SPLIT) {
      // (split launch with the policies fused: the rows also go to the LDS image the policy passes read)
      const int ln = (int)threadIdx.x & 63;
      if constexpr ((DUTY & DUTY_OBS0) != 0) {
        const RowsLdsT<WT ? AUX_WT : 0, OT> obl(ob, pol_lds_feat<POL_ROWS>(), 0, ln);
        env_obs<A, M, DUP, OT>(L, mp.R, slots, e, 0, p.cfg.obs.fow_radius, cfg_blind & 1, ego_blind, C, c0, c1, obl, 0);
        const double tsd = timestep_of(e.t, mp.R);   // (formed in place: held across the rows it costs registers)
        Out(p.timestep, p.n, 1, i, 8).st_f64(0, tsd);
        pol_lds_ts()[ln] = (float)tsd;
      }
      if constexpr ((DUTY & DUTY_OBS1) != 0) {
        const RowsLdsT<WT ? AUX_WT : 0, OT> obl(ob, pol_lds_feat<POL_ROWS>() + POL_ROWS * 64, F, ln);
        env_obs<A, M, DUP, OT>(L, mp.R, slots, e, 1, p.cfg.obs.fow_radius, (cfg_blind >> 1) & 1, ego_blind, C, c0, c1, obl, F);
      }
    } else {
      // (obp: the rows with this wave's offsets pre-formed, or plain rows where none were)
#ifdef OC_SPECIALIZED
      if constexpr (LN > 1) {
        if constexpr (DUTY == DUTY_OBS0) env_obs_lanes<A, M, DUP, OT, LN>(L, parts, e, 0, p.cfg.obs.fow_radius, C, c0, c1, obp, 0);
        if constexpr (DUTY == DUTY_OBS1) env_obs_lanes<A, M, DUP, OT, LN>(L, parts, e, 1, p.cfg.obs.fow_radius, C, c0, c1, obp, F);
      } else
#endif
      {
        if constexpr ((DUTY & DUTY_OBS0) != 0)
          env_obs<A, M, DUP, OT>(L, mp.R, slots, e, 0, p.cfg.obs.fow_radius, cfg_blind & 1, ego_blind, C, c0, c1, obp, 0);
        if constexpr ((DUTY & DUTY_OBS1) != 0)
          env_obs<A, M, DUP, OT>(L, mp.R, slots, e, 1, p.cfg.obs.fow_radius, (cfg_blind >> 1) & 1, ego_blind, C, c0, c1, obp, F);
      }
      // (a wave that does more than one viewer's rows: behind them, or the value would be held across both)
      if constexpr (TS_MINE && !OBS_ONLY) tso.st_f64(0, timestep_of(e.t, mp.R));
    }
    OC_STAMP(5);   // observation stores issued
    if constexpr (D_SHAPE) {
      // ... and they drain while the shaping is summed
      double s0, s1;
      shaping_sum<2>(L, sin, sq, s0, s1 OC_STAMP_PASS);
      const double shaped = ((double)reward - s0) - s1;  // :282
      Out(p.reward, p.n, 1, i, 8).st_f64(0, shaped);
      if (XO != 0 && p.opt.ep_return != nullptr) {   // uniform
        Out(p.opt.ep_return, p.n, 1, i, 8).st_f64(0, prev_done ? shaped : ep_ret + shaped);
        Out(p.opt.ep_length, p.n, 1, i).st(0, prev_done ? 1 : ep_len + 1);
      }
    }
  }
  OC_STAMP(7);   // every store issued
  if constexpr (D_STATE) slot.add(metrics_ != nullptr, valid, done, success, reward, comp, err);
  OC_STAMP(8);
  if constexpr (POL) {
    static_assert(XO != 0, "the fused policies belong to the variants with action sources");
    // split: every observation row (and the timestep) of this workgroup's 64 envs is in LDS;
    // a lone wave re-reads its own rows from memory
    if constexpr (SPLIT) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int lane = (int)threadIdx.x & 63;
    const Hdr L {maps.ref().L};
    const int C = p.cfg.obs.num_comm, F = 22 + L.S() + 2 * C;
    const uint32_t n32 = (uint32_t)n_;
    constexpr int ELEM = OT == 1 ? 1 : 4;
#pragma unroll
    for (int v = 0; v < 2; v++)
#pragma unroll
      for (int q = 0; q < 2; q++) {
        // a split workgroup: this wave's one pass (POL_MINE); a lone wave: all four
        if (SPLIT && (2 * v + q) != POL_MINE) continue;
        const int64_t env0 = (int64_t)(i & ~63) + 32 * q + (lane & 31);
        const bool ok = env0 < n_;
        const uint32_t env = (uint32_t)(ok ? env0 : n_ - 1);
        const void *rows = (const char *)p.obs + (size_t)v * F * n_ * ELEM;
        int32_t *pairs = (int32_t *)const_cast<void *>(v == 0 ? ego_src_ : alt_src_);
        if constexpr (SPLIT) {
          const int col = 32 * q + (lane & 31);
          ocpol::policy_pass<OT, 4, true, true>(rows, n32, env, ok, lane, p.pol[v].w1, p.pol[v].w2, p.pol[v].b2,
                                                p.pol[v].rng, pairs, nullptr, pol_lds_ts()[col], F, C, p.pol_ksteps,
                                                pol_lds_feat<POL_ROWS>() + v * POL_ROWS * 64, col, &pol_w);
        } else {
          ocpol::policy_pass<OT, 4>(rows, n32, env, ok, lane, p.pol[v].w1, p.pol[v].w2, p.pol[v].b2, p.pol[v].rng,
                                    pairs, nullptr, (float)p.timestep[env], F, C, p.pol_ksteps);
        }
      }
  }
#ifdef OC_STAMPS
  // the sparse-reward pointer doubles as the debug buffer in this build: int64 [waves][16]
  if ((threadIdx.x & 63) == 0 && p.sparse != nullptr) {   // one record per wave, split or not
    long long *dbg = (long long *)p.sparse + ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16;
    for (int k = 0; k < 16; k++) dbg[k] = (long long)oc_tt[k];
  }
#endif
}

// OvercookedMultiEnv.multi_step in one launch.  SP = waves per 64 envs: 1 = one wave does the
// whole step (block_ & 0xFFFF threads per workgroup); 4 = split launch, 256 threads per workgroup,
// the wave's index picks its duty (a uniform branch; each arm is its own instruction stream).
// The six leading scalars repeat fields of `p` (and the workgroup size, which would otherwise come
// from the hidden arguments): as plain leading arguments they are preloaded into SGPRs at wave
// launch (-mllvm -amdgpu-kernarg-preload-count, build.py), so the state and action loads are
// issued without first waiting for a scalar kernarg load.  (block_ = workgroup size | which
// optional action sources are in use << 16: the branches on them are taken on a preloaded SGPR,
// not on a pointer that a scalar load has yet to deliver; ego_src_ = opts.ego_pairs, alt_src_ =
// opts.alt_rng or opts.alt_pairs: preloaded as well (n_ is 32 bits wide so that the lot fits the
// 14 preloadable dwords), so the general variant issues its action loads with the state loads)
template <int M, bool LDS, int OT, bool WT, bool DUP, int XO, int SP, bool POL = false, int LN = 1>
__global__ void __launch_bounds__(256) k_multi_step(int32_t *const state_, const int32_t *const actions_,
                                                    int32_t *const comm_, int64_t *const metrics_,
                                                    const int32_t n_, const int32_t block_,
                                                    const void *const ego_src_, const void *const alt_src_,
                                                    const MultiArgs p) {
  static_assert(SP == 1 || SP == 2 || SP == 4, "waves per 64 envs");
  static_assert(SP != 2 || !POL, "the fused policies need the four-wave split");
  static_assert(SP == 1 || !LDS, "the split launch reads the tables from global memory");
  static_assert(LN == 1 || (SP == 4 && XO == 0 && !POL), "lanes per env: the plain four-way split only");
  OC_TL_BEGIN();
#ifdef OC_SPECIALIZED
  const MultiArgs &pk = p;
#else
  // Generic library: the split arms read the argument block through the kernarg segment pointer,
  // not through the by-value parameter.  With the body inlined four times the compiler no longer
  // forwarded `p` to the constant address space and kept a private copy instead -- 984 bytes of
  // scratch per lane here, where the header accessors index into the block dynamically (17 us per
  // step instead of 6.8; through the pointer 5.6).  The specialised libraries never had the copy
  // (tests/test_host_cpu.py checks every kernel of every built library) and keep the parameter:
  // loads through the pointer are not known to be invariant, and cost them 3 % (tomato-2) to 28 %
  // (a random-* level, whose map geometry is read at run time).
  struct KernArgs { int32_t *a; const int32_t *b; int32_t *c; int64_t *d; int32_t n, blk; const void *e, *f; MultiArgs p; };
  [[maybe_unused]] const MultiArgs &pk = *reinterpret_cast<const MultiArgs *>(
      reinterpret_cast<const char *>((const void *)__builtin_amdgcn_kernarg_segment_ptr()) + offsetof(KernArgs, p));
#endif
#define OC_BODY(duty) multi_step_body<M, LDS, OT, WT, DUP, XO, (duty), true, POL, LN>(state_, actions_, comm_, metrics_, n_, block_, ego_src_, alt_src_, pk, LaunchMap{{pk.L, pk.R, pk.tables, pk.n16}})
  if constexpr (SP == 1) {
    multi_step_body<M, LDS, OT, WT, DUP, XO, DUTY_ALL, false, POL>(state_, actions_, comm_, metrics_, n_, block_, ego_src_, alt_src_, p,
                                                                   LaunchMap{{p.L, p.R, p.tables, p.n16}});
  } else {
    const int role = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    if constexpr (SP == 2) {   // two waves per 64 envs: state + viewer 0 | shaping + viewer 1
      if (role == 0) OC_BODY(DUTY_STATE | DUTY_OBS0);
      else OC_BODY(DUTY_SHAPE | DUTY_OBS1);
    } else {
      // The waves of a workgroup do not start together: waves 2 and 3 came ~240 cycles after waves
      // 0 and 1 in every stamped run, and all four leave the barrier behind the state loads at the
      // time of the LAST one.  The two long arms (the observations: ~30 row stores each) therefore
      // go to the early waves, which at least issue their prologue under that wait, and the two
      // short arms to the late ones.
      if (role == 0) OC_BODY(DUTY_OBS0);
      else if (role == 1) OC_BODY(DUTY_OBS1);
      else if (role == 2) OC_BODY(DUTY_STATE);
      else OC_BODY(DUTY_SHAPE);
    }
  }
#undef OC_BODY
  OC_TL_END(p.timeline, p.timeline_stride, LN);
}


// ---------------------------------------------------------------------------
// map sets: envs on different maps of one structure in one launch
// ---------------------------------------------------------------------------
// Structure libraries only.  A map set is K maps of the library's structure and an assignment of
// every GROUP of 64 envs (64 g ... 64 g + 63) to one of them: group_map[g].  Nothing in the step needs
// a launch to share a map -- the geometry is a per-wave uniform value, read through the header's
// accessors -- so the kernels below are the single-level code (multi_step_body, obs_body, reset_body)
// handed the GROUP's header, run configuration and tables instead of the launch's:
//   - one device allocation holds the K records (MapRecord) and, behind them, the maps' table images;
//   - a workgroup always covers exactly one group (64 threads, or four duty waves over the same 64
//     envs), so its map is group_map[blockIdx.x]: one scalar load, then the record's words through
//     the CONSTANT address space -- scalar loads the compiler knows to be invariant, fetched where the
//     code first needs them (the first use is the pin behind the state and action loads: those are
//     issued from preloaded arguments and never wait for the record);
//   - state, observation rows, outputs and the metrics slots (one per wave of 64 envs = per group)
//     keep their layouts, so a map's counters are the sum of its groups' slots.
#if defined(OC_SPECIALIZED) && !defined(OC_SPEC_GEOMETRY)
struct MapRecord {
  LevelHdr L;        // (only the GEOMETRY fields are ever read: the structure is folded into the code)
  RunCfg R;          // inv_max_path is the map's; T and the ALLERGIC flags may differ as well
  int64_t tab_off;   // the map's table image (oc_level_host.h: build_tables): bytes from the first record,
  int32_t n16;       //   its size / 16
  int32_t pad_;
  const void *tables;   //   and its device address (the allocation's base + tab_off)
};

// the record of workgroup g's map, as seen through the constant address space
__device__ __forceinline__ const MapRecord &group_record(const MapRecord *maps, const int32_t *group_map, unsigned g) {
  typedef const __attribute__((address_space(4))) int32_t *ConstI32;
  typedef const __attribute__((address_space(4))) MapRecord *ConstRec;
  const int m = *((ConstI32)group_map + g);
  return *(const MapRecord *)((ConstRec)maps + m);
}
// The fused step's source of its map.  The lookup is two dependent scalar loads (group_map[g], then
// the record's words) behind the kernel arguments' own; it is ordered BEHIND the step's state and
// action loads -- a scheduling barrier, and the pointers passed through a statement the compiler
// cannot move -- so that the round trips run under the wait for the state.  (Left to the scheduler,
// the chain and its three waits went in front of the first vector load.)
struct GroupMap {
  const MapRecord *maps;
  const int32_t *group_map;
  __device__ __forceinline__ MapRef ref_behind_loads() const {
    __builtin_amdgcn_sched_barrier(0);
    const MapRecord *ms = maps;
    const int32_t *gm = group_map;
    asm volatile("" : "+s"(ms), "+s"(gm));
    const MapRecord &rec = group_record(ms, gm, blockIdx.x);
    // What the step pins under the wait for the state (multi_step_body) is fetched HERE, and the region
    // is closed: the scheduler otherwise moves the first arithmetic on loaded words -- and its wait for
    // the state -- in front of the record's loads, which then start a round trip of their own.
    asm volatile("" ::"s"(rec.tables), "s"(rec.R.inv_T), "s"(rec.R.inv_max_path), "s"(rec.L.W), "s"(rec.L.ncells),
                 "s"(rec.L.max_path), "s"(rec.L.cell_lo[0]), "s"(rec.L.cell_hi[0]), "s"(rec.L.deliv_pos[0]));
    __builtin_amdgcn_sched_barrier(0);
    return MapRef{rec.L, rec.R, rec.tables, rec.n16};
  }
};

struct SetMultiArgs {   // MultiArgs without the launch's map and without the fused policies
  const MapRecord *maps;
  const int32_t *group_map;
  void *obs;
  double *timestep;
  double *reward;
  int32_t *done;
  int32_t *sparse;
  const int32_t *placement;
  uint32_t *rng;
  oc_step_opts opt;
  int64_t n;
  int32_t auto_reset;
  oc_wrap_cfg cfg;
};

// The fused 2-agent step of a map set: XO = 0 / 1, one wave or four duty waves per 64 envs (SP = 1 /
// 4), write-through stores, tables in global memory.  Same leading (preloaded) scalars as
// k_multi_step; block_'s low half is always 64.
template <int M, int OT, bool DUP, int XO, int SP>
__global__ void __launch_bounds__(256) k_mapset_step(int32_t *const state_, const int32_t *const actions_,
                                                     int32_t *const comm_, int64_t *const metrics_,
                                                     const int32_t n_, const int32_t block_,
                                                     const void *const ego_src_, const void *const alt_src_,
                                                     const SetMultiArgs p) {
  static_assert(SP == 1 || SP == 4, "waves per 64 envs");
  static_assert(XO == 0 || XO == 1, "the wrapper's standard configuration");
  const GroupMap maps{p.maps, p.group_map};
#define OC_BODY(duty, split) multi_step_body<M, false, OT, true, DUP, XO, (duty), (split), false, 1>(state_, actions_, comm_, metrics_, n_, block_, ego_src_, alt_src_, p, maps)
  if constexpr (SP == 1) {
    OC_BODY(DUTY_ALL, false);
  } else {
    const int role = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // (the order: see k_multi_step)
    if (role == 0) OC_BODY(DUTY_OBS0, true);
    else if (role == 1) OC_BODY(DUTY_OBS1, true);
    else if (role == 2) OC_BODY(DUTY_STATE, true);
    else OC_BODY(DUTY_SHAPE, true);
  }
#undef OC_BODY
}

struct SetObsArgs {
  const MapRecord *maps;
  const int32_t *group_map;
  const int32_t *state;
  const int32_t *comm;
  void *obs;
  double *timestep;
  int64_t n;
  oc_obs_cfg cfg;
};

// oc_obs for a map set (the rows after a reset); 64 threads per workgroup
template <int M, int OT, bool DUP>
__global__ void __launch_bounds__(64) k_mapset_obs(const SetObsArgs p) {
  const MapRecord &rec = group_record(p.maps, p.group_map, blockIdx.x);
  obs_body<2, M, OT, true, DUP>(rec.L, rec.R, p);
}

struct SetResetArgs {
  const MapRecord *maps;
  const int32_t *group_map;
  int32_t *state;
  const int32_t *mask;
  const int32_t *placement;
  uint32_t *rng;
  int64_t n;
};

// oc_reset for a map set; 64 threads per workgroup
template <int M, bool DUP>
__global__ void __launch_bounds__(64) k_mapset_reset(const SetResetArgs p) {
  const MapRecord &rec = group_record(p.maps, p.group_map, blockIdx.x);
  reset_body<2, M, DUP>(rec.L, rec.tables, rec.n16, p);
}
#endif

}  // namespace
