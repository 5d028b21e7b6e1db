// X = 64, float64, per-graph tables: the "lean" scale-free sweep kernel (default path of BASELINE configs 2-4).
//
// Same algorithm and the same scale-free representation as sweep_x64_sf_kernel (mlbp_sweep.hip): one 256-thread
// workgroup owns one graph for all sweeps of a call, messages live in LDS carried with an exact power-of-two
// scale, the pairwise tables stay in registers, true normalisations (LBP.py:649-657) happen once after the last
// sweep, graphs the representation cannot hold are flagged for the exact kernel.  What differs is the cost of one
// update -- the old kernel spent ~275 wave instructions and ~10 dependent LDS round trips around 16 useful FMAs:
//
//   * the program is compiled on the host into 8-word micro-ops whose operands are LDS byte offsets, so an
//     update reads one descriptor and issues its message loads at once (no source lists, no slot arithmetic; the
//     list is padded with an all-ones slot, so two sources -- four with one branch -- are fetched without a count);
//   * a thread owns a 4 x 4 block of each table (rows 4R..4R+3, column pairs {2c,2c+1} and {32+2c,33+2c}), so BOTH
//     directions of an update are 16 FMAs followed by a short select-light reduction:
//        T.m   (reduce over columns): v_permlane16_swap (4 -> 2 values), one DPP step with a select (2 -> 1), two
//              plain DPP steps;
//        m^T.T (reduce over rows):    one DPP row_ror:8 step (the two column pairs sit in swapped registers in lanes
//              with bit 3 set, so no select is needed), v_permlane32_swap, then the four waves meet in LDS;
//     and the variable->factor product feeding an update is formed directly in the distribution the contraction
//     needs (4 columns or 4 rows per lane) -- no LDS round trip between product and contraction;
//   * every global load instruction of a table covers 128-byte contiguous pieces (8 lanes x 16 B).
// One barrier per bundle of (at most two independent) updates, as before.
#ifndef MLBP_LEAN_DEVICE_H
#define MLBP_LEAN_DEVICE_H

#include "mlbp_device.h"
#include "mlbp_uop.h"

using namespace mlbp_dev;

namespace {

constexpr int WG = 256;

// Per-graph pairwise tables are read once: non-temporal loads, 12.5 -> 13.0 k iterations/s on the default workload (R4.12; plain
// loads in their place cost 10-14 % on today's kernel, LAB_NOTES R32).  The unary rows stay plain loads.  An immediately
// invoked lambda: as a __forceinline__ function the same load leaves the kernels with a different register allocation.
typedef double nt_d2 __attribute__((ext_vector_type(2)));
#define NT_LOAD2(p) ([&] { const nt_d2 v_ = __builtin_nontemporal_load(reinterpret_cast<const nt_d2*>(p)); return make_double2(v_.x, v_.y); }())
// The X = 64 message write-back and the marginals of the first eight variables: written once, next read by another launch.
// Non-temporal stores: 2-3 % on the default workload (LAB_NOTES R32; no effect on the kernel of R4.12).
#define NT_STORE2(p, v) ([&] { nt_d2 x_; x_.x = (v).x; x_.y = (v).y; __builtin_nontemporal_store(x_, reinterpret_cast<nt_d2*>(p)); }())

constexpr int GROUP_WORDS = 48;     // one group descriptor of a MULTI launch (see launch_lean_groups)
// (micro-op words and the UOP_* bits of word 0: mlbp_internal.h, shared with build_lean_program in mlbp_compile.cpp)
using mlbp::UOP_VAR; using mlbp::UOP_MT; using mlbp::UOP_PSLOT_SHIFT; using mlbp::UOP_NOP; using mlbp::UOP_STORE_VF;
using mlbp::UOP_NSRC_SHIFT; using mlbp::UOP_CARRY_IN; using mlbp::UOP_CARRY_OUT;

struct LeanDev {
  const int32_t* image;   // bundles [n_bundles][16] | hoist [4][HL][2] | cprod lists [n_cprod][16] | written [4][WL] | pad
  const int32_t* readout; // [n_vars][16]: count, base slot, varying slots... (build_lean_readout) or NULL
  uint8_t* bail;          // [B]
  int32_t n_bundles, HL, n_cprod, WL, n_ext, init, dense, keep;
  int32_t walk;           // -1: workgroup i takes graph i; else the launch's last graph L, and workgroup i takes graph L - i: the
                          // launch walks the batch backward (mlbp_set_lean_walk)
};

// a' = [a.row0, b.row0, a.row2, b.row2], b' = [a.row1, b.row1, a.row3, b.row3] (rows of 16 lanes); a' + b'
__device__ __forceinline__ double swapadd16(double a, double b) {
  auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// a' = [a.lo32, b.lo32], b' = [a.hi32, b.hi32] (halves of 32 lanes); a' + b'
__device__ __forceinline__ double swapadd32(double a, double b) {
  auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

// The packed reductions (PACKED_NORM, PACKED_HOIST): the four DPP steps of wave_sum / wave_max_u32, which end with every lane of
// a row of 16 holding the row's total.  On a vector packed n consecutive entries to the lane, behind the in-lane adds, they are
// the tree's next four levels (lane ^ 1, lane ^ 2, the two mirrors pair the same partial sums as wave_sum's later steps do).
__device__ __forceinline__ double row16_sum(double v) {
  v += dpp_mov<0xB1>(v);
  v += dpp_mov<0x4E>(v);
  v += dpp_mov<0x141>(v);
  v += dpp_mov<0x140>(v);
  return v;
}
typedef int v4i __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v4i sload4(const int32_t* p) {      // four consecutive words through the scalar data cache, 16-byte aligned
  return *(const v4i __attribute__((address_space(4)))*)(uintptr_t)p;
}
__device__ __forceinline__ unsigned row16_max_u32(unsigned v) {
  v = max(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true));
  v = max(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true));
  v = max(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true));
  v = max(v, (unsigned)__builtin_amdgcn_mov_dpp((int)v, 0x140, 0xF, 0xF, true));
  return v;
}

// Workgroup-wide "any" with ONE barrier: each wave's ballot into its word of `votes`, the barrier, every thread reads the four
// words.  (__syncthreads_or / __syncthreads_and compile to three barriers each; the three votes of a launch cost 1.0-1.4 %
// of it that way.)  The four words must not be written again, by a later vote or as anything else, before every wave has
// passed one more barrier.
__device__ __forceinline__ bool vote_any(bool p, int32_t* votes, int wave, int lane) {
  const int mine = __ballot(p) != 0 ? 1 : 0;
  if (lane == 0) votes[wave] = mine;
  lds_barrier();
  const int4 v = *reinterpret_cast<const int4*>(votes);
  return (v.x | v.y | v.z | v.w) != 0;
}

struct LaneGeo {
  int tm0, tm1;   // byte offsets inside a message of the lane's column pairs held in table registers k = 0, 1
  int mt;         // byte offset of the lane's four rows
  int red_tm;     // byte offset (in a [64] array) of the row this lane reports after the T.m reduction
  int red_mt;     // byte offset (in a [4][64] array) of the column this lane reports after the m^T.T reduction
  bool up, st_tm, st_mt, wr_tm;
};

__device__ __forceinline__ double2 lds2(const char* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void mul2(double2& a, const double2 b) { a.x *= b.x; a.y *= b.y; }

// LDS by byte ADDRESS (the LDS_ADDR instances): an integer, formed from byte offsets by plain integer adds, cast once to an LDS
// pointer.  As `char* + offset` every access pays an add of the array's base -- a literal zero the compiler does not fold.
typedef double lds_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int lds_addr(const void* p) { return (int)(size_t)(const __attribute__((address_space(3))) char*)p; }
__device__ __forceinline__ double2 lds2_at(int a) {
  const lds_v2d v = *(const __attribute__((address_space(3))) lds_v2d*)(size_t)(unsigned)a;
  return make_double2(v.x, v.y);
}
__device__ __forceinline__ void lds2_put(int a, const double2 v) {
  lds_v2d w; w.x = v.x; w.y = v.y;
  *(__attribute__((address_space(3))) lds_v2d*)(size_t)(unsigned)a = w;
}
__device__ __forceinline__ double lds1_at(int a) { return *(const __attribute__((address_space(3))) double*)(size_t)(unsigned)a; }
__device__ __forceinline__ void lds1_put(int a, double v) { *(__attribute__((address_space(3))) double*)(size_t)(unsigned)a = v; }

// One table (T[r][k] = rows 4R + r, column pair k ^ b3) against one input vector; u = the micro-op's 8 words (scalars).
// u0 = flags (wave-uniform scalar); s1..s4, vf = source / store byte offsets (same in every lane, kept in VGPRs).
// A table held in registers, or -- the (NT+1)-th table of a 7-table graph -- in LDS as [r * 2 + k][thread] double2.
struct RegTable {
  const double2 (&T)[4][2];
  __device__ __forceinline__ double2 operator()(int r, int k) const { return T[r][k]; }
};
struct LdsTable {
  const double2* base;                      // this thread's column of the image
  __device__ __forceinline__ double2 operator()(int r, int k) const { return base[(r * 2 + k) * WG]; }
};

// WIDE: sources 3-4 are fetched together (else one after the other: the one-table instances, whose updates rarely have them,
// would pay eight registers and a fifth workgroup per CU for it)
template <bool MT, bool WIDE, typename TB>
__device__ __forceinline__ void contract(const TB T, char* wb, int u0, int s1, int s2, int s3, int s4, int vf,
                                         const LaneGeo& G, char* redA) {
  const int nsrc = (u0 >> UOP_NSRC_SHIFT) & 15;
  const bool has_vf = (u0 & UOP_STORE_VF) != 0;
  if (MT) {
    // sources 1-2 in one round trip, 3-4 in a second one: the host pads the list with the all-ones slot (x * 1.0 is exact)
    double2 ma = lds2(wb + s1 + G.mt), mb = lds2(wb + s1 + G.mt + 16);
    {
      const double2 a = lds2(wb + s2 + G.mt), b = lds2(wb + s2 + G.mt + 16);
      mul2(ma, a); mul2(mb, b);
    }
    if (nsrc > 2) {
      if (WIDE) {
        const double2 a2 = lds2(wb + s3 + G.mt), b2 = lds2(wb + s3 + G.mt + 16);
        const double2 a3 = lds2(wb + s4 + G.mt), b3 = lds2(wb + s4 + G.mt + 16);
        mul2(ma, a2); mul2(mb, b2);
        mul2(ma, a3); mul2(mb, b3);
      } else {
        mul2(ma, lds2(wb + s3 + G.mt)); mul2(mb, lds2(wb + s3 + G.mt + 16));
        if (nsrc > 3) { mul2(ma, lds2(wb + s4 + G.mt)); mul2(mb, lds2(wb + s4 + G.mt + 16)); }
      }
    }
    if (has_vf && G.st_mt) {
      *reinterpret_cast<double2*>(wb + vf + G.mt) = ma;
      *reinterpret_cast<double2*>(wb + vf + G.mt + 16) = mb;
    }
    double a00, a01, a10, a11;
    { const double2 t0 = T(0, 0), t1 = T(0, 1); a00 = ma.x * t0.x; a01 = ma.x * t0.y; a10 = ma.x * t1.x; a11 = ma.x * t1.y; }
    { const double2 t0 = T(1, 0), t1 = T(1, 1); a00 += ma.y * t0.x; a01 += ma.y * t0.y; a10 += ma.y * t1.x; a11 += ma.y * t1.y; }
    { const double2 t0 = T(2, 0), t1 = T(2, 1); a00 += mb.x * t0.x; a01 += mb.x * t0.y; a10 += mb.x * t1.x; a11 += mb.x * t1.y; }
    { const double2 t0 = T(3, 0), t1 = T(3, 1); a00 += mb.y * t0.x; a01 += mb.y * t0.y; a10 += mb.y * t1.x; a11 += mb.y * t1.y; }
    // rows: lane bit 3 (partner l ^ 8 keeps the other column pair in its register 0), lane bit 5, then the waves
    a00 += dpp_mov<0x128>(a10);
    a01 += dpp_mov<0x128>(a11);
    *reinterpret_cast<double*>(redA + G.red_mt) = swapadd32(a00, a01);
  } else {
    double2 m0 = lds2(wb + s1 + G.tm0), m1 = lds2(wb + s1 + G.tm1);
    {
      const double2 a = lds2(wb + s2 + G.tm0), b = lds2(wb + s2 + G.tm1);
      mul2(m0, a); mul2(m1, b);
    }
    if (nsrc > 2) {
      if (WIDE) {
        const double2 a2 = lds2(wb + s3 + G.tm0), b2 = lds2(wb + s3 + G.tm1);
        const double2 a3 = lds2(wb + s4 + G.tm0), b3 = lds2(wb + s4 + G.tm1);
        mul2(m0, a2); mul2(m1, b2);
        mul2(m0, a3); mul2(m1, b3);
      } else {
        mul2(m0, lds2(wb + s3 + G.tm0)); mul2(m1, lds2(wb + s3 + G.tm1));
        if (nsrc > 3) { mul2(m0, lds2(wb + s4 + G.tm0)); mul2(m1, lds2(wb + s4 + G.tm1)); }
      }
    }
    if (has_vf && G.st_tm) {
      *reinterpret_cast<double2*>(wb + vf + G.tm0) = m0;
      *reinterpret_cast<double2*>(wb + vf + G.tm1) = m1;
    }
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double2 t0 = T(r, 0), t1 = T(r, 1);
      v[r] = t0.x * m0.x;
      v[r] += t0.y * m0.y;
      v[r] += t1.x * m1.x;
      v[r] += t1.y * m1.y;
    }
    // columns: lane bit 4 (rows of 16 lanes exchange registers), lane bit 2 (select), lane bits 1 and 0 (plain)
    const double u0 = swapadd16(v[0], v[2]), u1 = swapadd16(v[1], v[3]);
    const double keep = G.up ? u1 : u0, send = G.up ? u0 : u1;
    double w = keep + dpp_mov<0x141>(send);
    w += dpp_mov<0xB1>(w);
    w += dpp_mov<0x4E>(w);
    *reinterpret_cast<double*>(redA + G.red_tm) = w;        // the four lanes of a quad hold (and store) the same row
  }
}

template <int NT, int NL>
__device__ __forceinline__ void front(const double2 (&tab)[NT][4][2], const double2* tl, char* wb, int u0, const int4& lo, const int4& hi,
                                      const LaneGeo& G, char* redA) {
  const int pslot = (u0 >> UOP_PSLOT_SHIFT) & 7;
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    if (p == pslot) {
      if (u0 & UOP_MT) contract<true, (NT > 1)>(RegTable{tab[p]}, wb, u0, lo.y, lo.z, lo.w, hi.x, hi.y, G, redA);
      else contract<false, (NT > 1)>(RegTable{tab[p]}, wb, u0, lo.y, lo.z, lo.w, hi.x, hi.y, G, redA);
    }
  }
  if (NL > 0 && pslot >= NT) {
    const LdsTable T = {tl + (size_t)(pslot - NT) * 8 * WG};
    if (u0 & UOP_MT) contract<true, (NT > 1)>(T, wb, u0, lo.y, lo.z, lo.w, hi.x, hi.y, G, redA);
    else contract<false, (NT > 1)>(T, wb, u0, lo.y, lo.z, lo.w, hi.x, hi.y, G, redA);
  }
}

// ---- the paired form of a bundle's front half (PAIR_GATHER instances): an update is a GATHER -- the product of its source
//      messages in the distribution the contraction needs, which depends on the direction only -- and a CONTRACTION of that
//      product with the selected table; both members gather before either contracts ----
struct Src { double2 a, b; };       // the lane's four entries of the product: T.m its two column pairs, m^T.T its four rows

// The gathers of BOTH members of a bundle as one piece of straight-line code: the members are independent, so the second
// one's LDS reads are in flight while the first one's products are formed, instead of behind its contraction.  uB may be the
// empty member (UOP_NOP: sources at offset 0, nothing stored, the product unused).  Products and stores are those of contract<>:
// ((s1 s2) s3) s4, no bit differs.
template <bool STORE_BRANCH, bool LDS_ADDR>
__device__ __forceinline__ void gather_pair(char* wb, int uA, const int4& A0, const int4& A1, int uB, const int4& B0, const int4& B1,
                                            const LaneGeo& G, Src& mA, Src& mB) {
  const bool mtA = (uA & UOP_MT) != 0, mtB = (uB & UOP_MT) != 0;
  const int a0 = mtA ? G.mt : G.tm0, a1 = mtA ? G.mt + 16 : G.tm1;
  const int b0 = mtB ? G.mt : G.tm0, b1 = mtB ? G.mt + 16 : G.tm1;
  auto rd = [&](int off) { return LDS_ADDR ? lds2_at(off) : lds2(wb + off); };
  auto wr = [&](int off, const double2 v) { if (LDS_ADDR) lds2_put(off, v); else *reinterpret_cast<double2*>(wb + off) = v; };
  mA.a = rd(A0.y + a0); mA.b = rd(A0.y + a1);
  mB.a = rd(B0.y + b0); mB.b = rd(B0.y + b1);
  {
    const double2 pa = rd(A0.z + a0), pb = rd(A0.z + a1);
    const double2 qa = rd(B0.z + b0), qb = rd(B0.z + b1);
    mul2(mA.a, pa); mul2(mA.b, pb);
    mul2(mB.a, qa); mul2(mB.b, qb);
  }
  // (sources 3-4: a member at a time, each under its own branch -- fetched together for both they would keep 48 registers
  // alive and spill the three-table instance)
  if (((uA >> UOP_NSRC_SHIFT) & 15) > 2) {
    const double2 pa = rd(A0.w + a0), pb = rd(A0.w + a1);
    const double2 ra = rd(A1.x + a0), rb = rd(A1.x + a1);
    mul2(mA.a, pa); mul2(mA.b, pb);
    mul2(mA.a, ra); mul2(mA.b, rb);
  }
  if (((uB >> UOP_NSRC_SHIFT) & 15) > 2) {
    const double2 qa = rd(B0.w + b0), qb = rd(B0.w + b1);
    const double2 sa = rd(B1.x + b0), sb = rd(B1.x + b1);
    mul2(mB.a, qa); mul2(mB.b, qb);
    mul2(mB.a, sa); mul2(mB.b, sb);
  }
  if (STORE_BRANCH) {
    // the wave-uniform flag first, as a scalar branch: two members in three store nothing, and pay no lane predicate for it
    // (the empty asm keeps the compiler from folding the two conditions back into one lane mask; the lane predicate -- G.st_mt,
    // G.st_tm -- straight from the thread index, so that nothing of it is prepared ahead of the branch)
    const int t = threadIdx.x;
    auto mine = [&](bool mt) { return (t & (mt ? 0x17 : 0xE8)) == 0; };        // (0xE8: lane bits 3 and 5 clear, in wave 0)
    if (uA & UOP_STORE_VF) {
      asm volatile("");
      if (mine(mtA)) { wr(A1.y + a0, mA.a); wr(A1.y + a1, mA.b); }
    }
    if (uB & UOP_STORE_VF) {
      asm volatile("");
      if (mine(mtB)) { wr(B1.y + b0, mB.a); wr(B1.y + b1, mB.b); }
    }
    return;
  }
  if ((uA & UOP_STORE_VF) && (mtA ? G.st_mt : G.st_tm)) { wr(A1.y + a0, mA.a); wr(A1.y + a1, mA.b); }
  if ((uB & UOP_STORE_VF) && (mtB ? G.st_mt : G.st_tm)) { wr(B1.y + b0, mB.a); wr(B1.y + b1, mB.b); }
}

// (every sum is spelled out, with contraction off: the SECOND product rounded on its own, then the first, third and fourth fused
// onto it -- the form the compiler gave `a * b + c * d + ...` while each direction formed its own products.  Left to it, which
// product of a sum is rounded alone is its choice, and it changes when the two directions share a product, as they do behind
// one gather: a result would depend on the instance that computed it)
template <bool MT, typename TB>
__device__ __forceinline__ void contract_gathered(const TB T, const Src m, const LaneGeo& G, char* redA) {
#pragma clang fp contract(off)
  if (MT) {
    const double2 ma = m.a, mb = m.b;
    double a00, a01, a10, a11;
    { const double2 t0 = T(1, 0), t1 = T(1, 1); a00 = ma.y * t0.x; a01 = ma.y * t0.y; a10 = ma.y * t1.x; a11 = ma.y * t1.y; }
#define MLBP_ROW(mv, r) { const double2 t0 = T(r, 0), t1 = T(r, 1); a00 = __builtin_fma(mv, t0.x, a00); a01 = __builtin_fma(mv, t0.y, a01); \
                          a10 = __builtin_fma(mv, t1.x, a10); a11 = __builtin_fma(mv, t1.y, a11); }
    MLBP_ROW(ma.x, 0)
    MLBP_ROW(mb.x, 2)
    MLBP_ROW(mb.y, 3)
#undef MLBP_ROW
    // rows: lane bit 3 (partner l ^ 8 keeps the other column pair in its register 0), lane bit 5, then the waves
    a00 += dpp_mov<0x128>(a10);
    a01 += dpp_mov<0x128>(a11);
    *reinterpret_cast<double*>(redA + G.red_mt) = swapadd32(a00, a01);
  } else {
    const double2 m0 = m.a, m1 = m.b;
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double2 t0 = T(r, 0), t1 = T(r, 1);
      v[r] = t0.y * m0.y;
      v[r] = __builtin_fma(t0.x, m0.x, v[r]);
      v[r] = __builtin_fma(t1.x, m1.x, v[r]);
      v[r] = __builtin_fma(t1.y, m1.y, v[r]);
    }
    // columns: lane bit 4 (rows of 16 lanes exchange registers), lane bit 2 (select), lane bits 1 and 0 (plain)
    const double u0 = swapadd16(v[0], v[2]), u1 = swapadd16(v[1], v[3]);
    const double keep = G.up ? u1 : u0, send = G.up ? u0 : u1;
    double w = keep + dpp_mov<0x141>(send);
    w += dpp_mov<0xB1>(w);
    w += dpp_mov<0x4E>(w);
    *reinterpret_cast<double*>(redA + G.red_tm) = w;        // the four lanes of a quad hold (and store) the same row
  }
}

template <int NT>
__device__ __forceinline__ void front_gathered(const double2 (&tab)[NT][4][2], int u0, const Src m, const LaneGeo& G, char* redA) {
  const int pslot = (u0 >> UOP_PSLOT_SHIFT) & 7;
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    if (p == pslot) {
      if (u0 & UOP_MT) contract_gathered<true>(RegTable{tab[p]}, m, G, redA);
      else contract_gathered<false>(RegTable{tab[p]}, m, G, redA);
    }
  }
}

// FactorGraph.get_unregularized_gradeint (LBP.py:301-320) for one graph, from what the workgroup still holds after its
// sweeps: tables in registers (4 x 4 blocks), messages in LDS.  Pairwise factor (LBP.py:543-569, 592-619): beliefs =
// normalize((c r^T) (.) T), gradient = phi[label cell] - sum_ij beliefs_ij phi_ij -- the scale of c and r cancels, so the
// scaled messages serve as they are, and the 64 x 64 belief matrix is never formed: each thread folds its 16 cells into
// Z and three feature sums.  Unary factor (LBP.py:535-541, 600-603): beliefs = au.normalize(table), which IS the factor's
// hoisted message whenever the table's total is positive (else zero); its expected features are accumulated per lane over
// the wave's factors and reduced once.  gst: [U] message slot, [U] total positive, [U] kind, [U] observed column, [U] label.
template <int NT>
__device__ __forceinline__ void gradient_epilogue(const SweepDev& d, const GradFusedDev& gf, const double2 (&tab)[NT][4][2],
                                                  const char* wb, const int32_t* gst, double* scratch, const LaneGeo& G, int g,
                                                  int R_, int c_, int b3_) {
  constexpr int FEE = 3, FED = 6;
  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  // Pairwise factors.  sum_p E_p[k] = sum_ij (sum_p b_p[i][j]) phi[i][j][k] over the factors p that read one feature tensor, b_p =
  // the factor's normalised beliefs: so the beliefs of those factors are ADDED cell by cell first and the tensor -- 98 KB per
  // graph out of L2, interleaved [64][64][3] -- goes past once per graph instead of once per factor (2.4 GB per 8192-graph
  // launch of K3 graphs: what the epilogue was bound by).  Three steps, all on the thread's 4 x 4 blocks:
  //   1. W_p = (c r^T) (.) T_p in place of the table registers, and its total Z_p (wave sums, the four waves meet in LDS);
  //   2. V_t = sum over the factors reading tensor t (gap == 1: phi_en_en_w1, else phi_en_en; LBP.py:469-480) of W_p / Z_p
  //      (au.normalize: a total <= 0 gives zero beliefs);
  //   3. G_t[k] = sum_ij V_t[i][j] phi_t[i][j][k]: three accumulators per tensor, the thread's sixteen cells of the tensor
  //      loaded eight at a time.
  // thread p < P: the label cell's features of pairwise factor p -- two dependent loads, requested first and long finished when
  // thread 0 adds them up (they used to be the last thing the workgroup waited for, one thread, two round trips)
  double lf[FEE] = {0.0, 0.0, 0.0};
  bool lbad = false;
  if (t < NT && t < d.P) {
    const int l0 = gf.pair_label[((size_t)g * d.P + t) * 2], l1 = gf.pair_label[((size_t)g * d.P + t) * 2 + 1];
    if ((unsigned)l0 >= 64u || (unsigned)l1 >= 64u) lbad = true;
    else {
      const double* phl = (gf.pair_phi[t] ? gf.phi_en_en_w1 : gf.phi_en_en) + ((size_t)l0 * 64 + l1) * FEE;
#pragma unroll
      for (int q = 0; q < FEE; ++q) lf[q] = phl[q];
    }
  }
  int which = 0;                                                 // bit p: factor p reads phi_en_en_w1
  double2 W[NT][4][2];
  double* zs = scratch + 512;                                    // [4 waves][NT] (the per-wave results below use scratch[0 .. 4 PER))
  double* lfs = scratch + 544;                                   // [NT][FEE] the label features, for thread 0's final sum
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    double z = 0.0;
    if (p < d.P) {
      const int cs = as_const(gf.pair_c_slot)[p], rs = as_const(gf.pair_r_slot)[p];
      which |= (as_const(gf.pair_phi)[p] ? 1 : 0) << p;
      const double2 ca = lds2(wb + cs * 512 + G.mt), cb = lds2(wb + cs * 512 + G.mt + 16);
      const double2 r0 = lds2(wb + rs * 512 + G.tm0), r1 = lds2(wb + rs * 512 + G.tm1);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double ci = r == 0 ? ca.x : (r == 1 ? ca.y : (r == 2 ? cb.x : cb.y));
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const double2 rj = k ? r1 : r0, T = tab[p][r][k];
          W[p][r][k] = make_double2((ci * rj.x) * T.x, (ci * rj.y) * T.y);
          z += W[p][r][k].x + W[p][r][k].y;
        }
      }
      z = wave_sum(z);
      if (lane == 0) zs[wave * NT + p] = z;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) W[p][r][0] = W[p][r][1] = make_double2(0.0, 0.0);
    }
  }
  if (lbad) atomicExch(d.status, 1);
  if (t < NT && t < d.P) {                                       // (parked in LDS here: kept in registers to the end they spill the tables)
#pragma unroll
    for (int q = 0; q < FEE; ++q) lfs[t * FEE + q] = lf[q];
  }
  lds_barrier();
  double2 V[2][4][2];
#pragma unroll
  for (int tz = 0; tz < 2; ++tz)
#pragma unroll
    for (int r = 0; r < 4; ++r) V[tz][r][0] = V[tz][r][1] = make_double2(0.0, 0.0);
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    if (p < d.P) {
      const double Z = (zs[p] + zs[NT + p]) + (zs[2 * NT + p] + zs[3 * NT + p]);
      const double inv = Z > 0.0 ? 1.0 / Z : 0.0;                // au.normalize: zero sum -> zero beliefs
      const double i0 = ((which >> p) & 1) ? 0.0 : inv, i1 = ((which >> p) & 1) ? inv : 0.0;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          V[0][r][k].x += W[p][r][k].x * i0; V[0][r][k].y += W[p][r][k].y * i0;
          V[1][r][k].x += W[p][r][k].x * i1; V[1][r][k].y += W[p][r][k].y * i1;
        }
    }
  }
  double gacc[2][FEE] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  const int all = (1 << (d.P < NT ? d.P : NT)) - 1;
#pragma unroll
  for (int tz = 0; tz < 2; ++tz) {
    if (tz ? (which & all) == 0 : (which & all) == all) continue;          // no factor reads this tensor (wave-uniform)
    // (global address space spelled out: behind a run-time choice the loads otherwise come out as FLAT ones, which wait on
    // the LDS counter as well)
    typedef double v2d __attribute__((ext_vector_type(2)));
    typedef const v2d __attribute__((address_space(1))) * gptr2;
    const double* phi = tz ? gf.phi_en_en_w1 : gf.phi_en_en;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int col = 32 * (k ? 1 - b3_ : b3_) + 2 * c_;
      v2d cell[4][3];                                            // cell (i, col): f0 f1 f2 | cell (i, col + 1): g0 g1 g2
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const gptr2 ph = (gptr2)(uintptr_t)(phi + ((size_t)(4 * R_ + r) * 64 + col) * FEE);   // 48 bytes, 16-aligned
        cell[r][0] = ph[0]; cell[r][1] = ph[1]; cell[r][2] = ph[2];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double w0 = V[tz][r][k].x, w1 = V[tz][r][k].y;
        gacc[tz][0] += w0 * cell[r][0].x + w1 * cell[r][1].y;
        gacc[tz][1] += w0 * cell[r][0].y + w1 * cell[r][2].x;
        gacc[tz][2] += w0 * cell[r][1].x + w1 * cell[r][2].y;
      }
    }
  }
  double gsum[FEE];                                              // expected features of all pairwise factors (this wave's share)
#pragma unroll
  for (int q = 0; q < FEE; ++q) gsum[q] = wave_sum(gacc[0][q] + gacc[1][q]);
  // unary factors: wave w takes factors w, w + 4, ...; six at a time so that their feature slabs are in flight together (the
  // tables are dead by now: the registers are there)
  double lab_ee[FEE] = {0.0, 0.0, 0.0}, lab_ed[FED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // phi at the label (wave-uniform)
  double exp_ee[FEE] = {0.0, 0.0, 0.0}, exp_ed[FED] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};     // per-lane partial expected features
  bool bad = false;
  constexpr int UB = 6;                                          // (a K3 user graph's 24 unary factors: one round trip per wave)
  const int U = d.U;
  for (int u0 = wave; u0 < U; u0 += 4 * UB) {
    double b[UB], pv[UB][FED];
    int kd[UB], at[UB];
#pragma unroll
    for (int j = 0; j < UB; ++j) {
      const int u = u0 + 4 * j;
      kd[j] = -1;
      if (u < U) {
        const int kind = __builtin_amdgcn_readfirstlane(gst[2 * U + u]), obs = __builtin_amdgcn_readfirstlane(gst[3 * U + u]);
        const int lab = __builtin_amdgcn_readfirstlane(gst[4 * U + u]);
        const int cols = kind == 2 ? gf.Vde : 64;
        if ((unsigned)obs >= (unsigned)cols || (unsigned)lab >= 64u || (unsigned)kind > 2u) { bad = true; continue; }
        kd[j] = kind;
        const int slot = __builtin_amdgcn_readfirstlane(gst[u]);
        b[j] = __builtin_amdgcn_readfirstlane(gst[U + u]) ? *reinterpret_cast<const double*>(wb + slot * 512 + lane * 8) : 0.0;
        if (kind == 2) {
          const double2* ph = reinterpret_cast<const double2*>(gf.phi_en_de_t + ((size_t)obs * 64 + lane) * FED);
          at[j] = (obs * 64 + lab) * FED;
          const double2 a0 = ph[0], a1 = ph[1], a2 = ph[2];
          pv[j][0] = a0.x; pv[j][1] = a0.y; pv[j][2] = a1.x; pv[j][3] = a1.y; pv[j][4] = a2.x; pv[j][5] = a2.y;
        } else {
          typedef const double __attribute__((address_space(1))) * gptr1;      // (global, not FLAT, behind the run-time choice of tensor)
          const gptr1 ph = (gptr1)(uintptr_t)((kind ? gf.phi_en_en_w1_t : gf.phi_en_en_t) + ((size_t)obs * 64 + lane) * FEE);
          at[j] = (obs * 64 + lab) * FEE;
#pragma unroll
          for (int q = 0; q < FEE; ++q) pv[j][q] = ph[q];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < UB; ++j) {
      if (kd[j] == 2) {
#pragma unroll
        for (int q = 0; q < FED; ++q) { lab_ed[q] += as_const_f64(gf.phi_en_de_t)[at[j] + q]; exp_ed[q] += b[j] * pv[j][q]; }
      } else if (kd[j] >= 0) {
        const double* base = kd[j] ? gf.phi_en_en_w1_t : gf.phi_en_en_t;
#pragma unroll
        for (int q = 0; q < FEE; ++q) { lab_ee[q] += as_const_f64(base)[at[j] + q]; exp_ee[q] += b[j] * pv[j][q]; }
      }
    }
  }
  if (bad && lane == 0) atomicExch(d.status, 1);
  // combine the four waves: per wave the FEE pairwise sums, then FEE + FED unary sums
  constexpr int PER = FEE + FEE + FED;
  {
    double ue[FEE], ud[FED];
#pragma unroll
    for (int q = 0; q < FEE; ++q) ue[q] = lab_ee[q] - wave_sum(exp_ee[q]);
#pragma unroll
    for (int q = 0; q < FED; ++q) ud[q] = lab_ed[q] - wave_sum(exp_ed[q]);
    if (lane == 0) {
      double* o = scratch + wave * PER;
#pragma unroll
      for (int q = 0; q < FEE; ++q) o[q] = gsum[q];
#pragma unroll
      for (int q = 0; q < FEE; ++q) o[FEE + q] = ue[q];
#pragma unroll
      for (int q = 0; q < FED; ++q) o[FEE + FEE + q] = ud[q];
    }
  }
  lds_barrier();
  if (t == 0) {
    double tot[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) tot[q] = (scratch[q] + scratch[PER + q]) + (scratch[2 * PER + q] + scratch[3 * PER + q]);
    double gee[FEE];
#pragma unroll
    for (int q = 0; q < FEE; ++q) gee[q] = tot[FEE + q] - tot[q];
#pragma unroll
    for (int p = 0; p < NT; ++p) {
      if (p < d.P) {
#pragma unroll
        for (int q = 0; q < FEE; ++q) gee[q] += lfs[p * FEE + q];
      }
    }
#pragma unroll
    for (int q = 0; q < FEE; ++q) gf.grad_en_en[(size_t)g * FEE + q] = gee[q];
#pragma unroll
    for (int q = 0; q < FED; ++q) gf.grad_en_de[(size_t)g * FED + q] = tot[FEE + FEE + q];
  }
}

// The 64 partial results of one update (lane = state), rescaled by an exact power of two so that ONE normal element
// lands in [1, 2) (the first one; which one is immaterial -- the scale cancels in everything normalised later).
// `bad` is raised when the vector cannot be carried this way: a negative / non-finite entry, or no normal entry at all
// (the zero-sum -> uniform rule of LBP.py:655-657 would act).  No branch: a bad graph keeps computing (harmlessly) and
// is handed to the exact kernel when its sweeps are over.
__device__ __forceinline__ double rescale(double r, int& bad) {
  const unsigned key = mag_key(r);
  const unsigned long long normal = __ballot(key - KEY_MIN < KEY_BAD - KEY_MIN);
  const unsigned long long wrong = __ballot(key >= KEY_BAD);
  bad |= (wrong != 0) | (normal == 0);
  const int ref = __builtin_amdgcn_readlane((int)key, normal ? __builtin_ctzll(normal) : 0);
  return __builtin_ldexp(r, 1023 - ((ref >> 20) & 0x7FF));
}

// The same with the "negative or non-finite" half of the verdict left to the caller: the lane's largest key so far goes into
// `kmax`, to be looked at once behind the loop -- an OR over updates and lanes of `key >= KEY_BAD` IS `max(key) >= KEY_BAD`.  "No
// normal entry" stays per update: its ballot picks the reference lane anyway, and its share of the verdict stays on the scalar
// side -- `some` (start: all ones) is the minimum over the updates of the ballot's two halves OR-ed, zero once a ballot was empty.
__device__ __forceinline__ double rescale_kmax(double r, unsigned& some, unsigned& kmax) {
  const unsigned key = mag_key(r);
  const unsigned long long normal = __ballot(key - KEY_MIN < KEY_BAD - KEY_MIN);
  kmax = max(kmax, key);
  some = min(some, (unsigned)normal | (unsigned)(normal >> 32));
  const int ref = __builtin_amdgcn_readlane((int)key, normal ? __builtin_ctzll(normal) : 0);
  return __builtin_ldexp(r, 1023 - ((ref >> 20) & 0x7FF));
}

#ifdef MLBP_LEAN_STATIC
// ---- the static form of the main loop (sweep_x64_lean_static_kernel).  MLBP_LEAN_STATIC_IMAGE: the bundle words of ONE
//      program's image ([MLBP_LEAN_STATIC_BUNDLES][16], comma separated), known when the kernel is compiled.  Bundle K is
//      StaticBundle<K>::run, which ends by calling bundle K + 1 -- recursion, because no loop is unrolled across the barrier's asm.
//      A step is the interpreter's loop body with constant words: the same helpers in the same order, so no bit of a result
//      differs; what is gone is the fetch of the words, the decoding of the flags and the adds of slot offsets, which reach the
//      LDS instructions as their immediate offsets ----
constexpr int32_t STATIC_IMAGE[] = {MLBP_LEAN_STATIC_IMAGE};
constexpr int STATIC_BUNDLES = MLBP_LEAN_STATIC_BUNDLES;
static_assert(sizeof(STATIC_IMAGE) == sizeof(int32_t) * 16 * STATIC_BUNDLES, "the image is [bundles][16]");
// the half of `red` bundle k writes: the number of contraction bundles ahead of it, modulo 2
constexpr int static_parity(int k) {
  int p = 0;
  for (int j = 0; j < k; ++j) p ^= (STATIC_IMAGE[16 * j] & UOP_VAR) ? 0 : 1;
  return p;
}
struct StaticCtx {
  char* wb;
  char* red;
  const LaneGeo& G;
  int lane8, lane;
};
template <int K>
struct StaticBundle {
  static __device__ __forceinline__ void run(const StaticCtx& c, const double2 (&tab)[3][4][2], unsigned& some, unsigned& kmax) {
    constexpr int o = 16 * K;
    constexpr int fA = STATIC_IMAGE[o], fB = STATIC_IMAGE[o + 8];
    constexpr int a1 = STATIC_IMAGE[o + 1], a2 = STATIC_IMAGE[o + 2], a3 = STATIC_IMAGE[o + 3], a4 = STATIC_IMAGE[o + 4];
    constexpr int a5 = STATIC_IMAGE[o + 5], a6 = STATIC_IMAGE[o + 6];
    constexpr int b1 = STATIC_IMAGE[o + 9], b2 = STATIC_IMAGE[o + 10], b3 = STATIC_IMAGE[o + 11], b4 = STATIC_IMAGE[o + 12];
    constexpr int b5 = STATIC_IMAGE[o + 13], b6 = STATIC_IMAGE[o + 14];
    if constexpr ((fA & UOP_VAR) != 0) {
      constexpr int nsrc = (fA >> UOP_NSRC_SHIFT) & 15;
      double m = lds1_at(a1 + c.lane8);
      const double m2 = lds1_at(a2 + c.lane8);
      // (no carry links: a variable of a three-table graph multiplies at most four sources; lean_jit_specialize refuses a
      // program that holds one)
      static_assert((fA & (UOP_CARRY_IN | UOP_CARRY_OUT)) == 0, "the static step has no arm for carry links");
      m *= m2;
      if constexpr (nsrc > 2) {
        const double m3 = lds1_at(a3 + c.lane8);
        const double m4 = lds1_at(a4 + c.lane8);
        m *= m3;
        m *= m4;
      }
      lds1_put(a5 + c.lane8, m);
    } else {
      char* redP = c.red + static_parity(K) * 4096;
      constexpr bool two = !(fB & UOP_NOP);
      const int4 A0 = make_int4(fA, a1, a2, a3), A1 = make_int4(a4, a5, a6, 0);
      const int4 B0 = make_int4(fB, b1, b2, b3), B1 = make_int4(b4, b5, b6, 0);
      Src mA, mB;
      gather_pair<true, true>(c.wb, fA, A0, A1, fB, B0, B1, c.G, mA, mB);
      front_gathered<3>(tab, fA, mA, c.G, redP);
      if constexpr (two) front_gathered<3>(tab, fB, mB, c.G, redP + 2048);
      lds_barrier();
      const double* rd = reinterpret_cast<const double*>(redP);
      double rA = rd[c.lane];
      if constexpr ((fA & UOP_MT) != 0) rA = (rA + rd[64 + c.lane]) + (rd[128 + c.lane] + rd[192 + c.lane]);
      lds1_put(a6 + c.lane8, rescale_kmax(rA, some, kmax));
      // (kmax is taken now: in straight-line code the compiler otherwise puts every update's max off to the end of the loop and
      // keeps all their keys in registers until then -- a program of fourteen bundles spills)
      asm volatile("" : "+v"(kmax));
      if constexpr (two) {
        double rB = rd[256 + c.lane];
        if constexpr ((fB & UOP_MT) != 0) rB = (rB + rd[320 + c.lane]) + (rd[384 + c.lane] + rd[448 + c.lane]);
        lds1_put(b6 + c.lane8, rescale_kmax(rB, some, kmax));
        asm volatile("" : "+v"(kmax));
      }
    }
    StaticBundle<K + 1>::run(c, tab, some, kmax);
  }
};
template <>
struct StaticBundle<STATIC_BUNDLES> {
  static __device__ __forceinline__ void run(const StaticCtx&, const double2 (&)[3][4][2], unsigned&, unsigned&) {}
};
#endif

// PADX: X = d.X < 64 states, vectors and tables zero-padded to 64 on the way in, the first X entries written back.
// MULTI: the launch holds several GROUPS of graphs -- each group its own program (topology and root sequence), tables,
// messages -- described by a device table; the workgroup looks its group up and from then on runs as if launched for
// that group alone.  This is what lets a minibatch of mixed sentence shapes, each with its own roots (LBP.py:223-225,
// train_mp.py:257-299), sweep in one launch.
// NL: tables NT .. NT+NL-1 of the graph live in LDS instead of registers (a 7-table chain then fits 242 VGPRs + 70 KB, so two
// workgroups share a CU, where 8 register-resident tables allow one).
// GRAD: FactorGraph.get_unregularized_gradeint (LBP.py:301-320) of the graph as an epilogue (gradient_epilogue): the tables
// are still in registers and the messages in LDS, so the per-graph gradient costs no second pass over the tables in HBM.
// One body under two heads.  A build with MLBP_LEAN_STATIC defined (at run time, mlbp_lean_jit.cpp) compiles it ONCE, as
// sweep_x64_lean_static_kernel: the <3, false, false, 0, false> instance whose main loop is the expansion of a compile-time image
// (StaticBundle) instead of the interpreter of the image in memory; everything around the loop is the same text.  (A device
// function called from two kernels would be one text too, but the instances then come out with other instruction streams.)
// The static kernel is no kernel of libmlbp.so: it exists only in modules compiled at run time, and the translation unit that
// is compiled then (static_source, mlbp_lean_jit.cpp) brings its declarator -- MLBP_LEAN_STATIC_ENTRY: extern "C", the launch
// bounds (WG, 3), the name sweep_x64_lean_static_kernel, the parameters (SweepDev d, LeanDev f) -- along with the program's words.
#ifdef MLBP_LEAN_STATIC
MLBP_LEAN_STATIC_ENTRY {
  constexpr int NT = 3, NL = 0;
  constexpr bool PADX = false, MULTI = false, GRAD = false, STATIC = true;
  const int32_t* const groups = nullptr;
  const int n_groups = 0;
  const GradFusedDev gf = {};
#else
template <int NT, bool PADX, bool MULTI, int NL, bool GRAD>
// (GRAD instances: two workgroups per CU -- the epilogue keeps twelve accumulators and a thread's cells of a feature tensor beside
// the tables, which does not fit the 168 registers of three; the sweeps lose nothing at two per CU, profiles/r03h_lean_kernel_occupancy.txt)
__global__ __launch_bounds__(WG, (NT >= 7 ? 1 : (NT >= 4 ? 2 : 3))) void sweep_x64_lean_kernel(SweepDev d, LeanDev f, const int32_t* groups,
                                                                                             int n_groups, GradFusedDev gf) {
  constexpr bool STATIC = false;
#endif
  // (a workgroup owns its graph and reads no other's: which one it takes changes the order the batch streams in, and no result.
  // Ahead of the group look-up, so a grouped launch is reversed as a whole)
  int g = f.walk < 0 ? (int)blockIdx.x : f.walk - (int)blockIdx.x;
  if (MULTI) {
    // groups[k * GROUP_WORDS] = first graph of group k (ascending): the last k with start <= g
    int lo = 0, hi = n_groups - 1;
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (as_const(groups)[(size_t)mid * GROUP_WORDS] <= g) lo = mid; else hi = mid - 1;
    }
    const int32_t* G = groups + (size_t)lo * GROUP_WORDS;
    const Words16 w0 = sload16(G), w1 = sload16(G + 16), w2 = sload16(G + 32);
    auto ptr = [](int32_t a, int32_t b) { return (uintptr_t)(uint32_t)a | ((uintptr_t)(uint32_t)b << 32); };
    g -= w0.w[0];
    f.image = (const int32_t*)ptr(w0.w[2], w0.w[3]); f.readout = (const int32_t*)ptr(w0.w[4], w0.w[5]);
    f.bail = (uint8_t*)ptr(w0.w[6], w0.w[7]); d.msgs = (double*)ptr(w0.w[8], w0.w[9]);
    d.marginals = (double*)ptr(w0.w[10], w0.w[11]); d.pair_tables = (const double*)ptr(w0.w[12], w0.w[13]);
    d.pair_tab = (const int32_t*)ptr(w0.w[14], w0.w[15]); d.unary_tables = (const double*)ptr(w1.w[0], w1.w[1]);
    d.unary_tab = (const int32_t*)ptr(w1.w[2], w1.w[3]); d.status = (int32_t*)ptr(w1.w[4], w1.w[5]);
    f.n_bundles = w1.w[6]; f.HL = w1.w[7]; f.n_cprod = w1.w[8]; f.WL = w1.w[9]; f.n_ext = w1.w[10];
    d.n_msgs = w1.w[11]; d.P = w1.w[12]; d.U = w1.w[13]; d.n_vars = w1.w[14]; d.n_pair_tables = w1.w[15];
    d.n_unary_tables = w2.w[0]; f.dense = w2.w[1];
  }
  extern __shared__ double lds[];
  double* work = lds;                                        // [n_msgs + n_ext][64] scaled messages
  double* red = lds + (size_t)(d.n_msgs + f.n_ext) * 64;     // [2 parities][2 bundle slots][4][64]
  int32_t* limg = reinterpret_cast<int32_t*>(red + 4 * 256);      // [n_bundles + 1][16] micro-ops
  double2* tl = reinterpret_cast<double2*>(limg + 16 * (f.n_bundles + 1));      // [NL][8][256] tables kept in LDS
  // GRAD: per unary factor -- message slot, table total positive?, kind, observed column, label
  int32_t* gst = reinterpret_cast<int32_t*>(tl + (size_t)NL * 8 * WG);

  const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int X = PADX ? d.X : 64;
  const double uniform = 1.0 / (double)X;
  const double uni_l = (!PADX || lane < X) ? uniform : 0.0;      // the uniform vector, lane = state
  double* gm = d.msgs + (size_t)g * d.n_msgs * X;
  const int32_t* img_hoist = f.image + 16 * (size_t)f.n_bundles;
  const int32_t* img_cprod = img_hoist + 8 * (size_t)f.HL;
  const int32_t* img_written = img_cprod + 16 * (size_t)f.n_cprod;
  // the words of the workgroup votes (vote_any) lie in red, idle outside the sweeps: the first and the last vote at its start
  // (next written by the first bundle, behind the second vote's barrier; after the last vote by the gradient epilogue, behind
  // its own barrier), the second vote, which leads straight into the sweeps, in the half the SECOND bundle writes
  int32_t* votes = reinterpret_cast<int32_t*>(red);
  // (the GRAD instances keep the library's votes and the micro-ops' own barrier: they sit at their register limit, and this
  // form costs them two more spilled registers and 2.4 % of the train step)
  constexpr bool LEAN_SYNC = !GRAD;
  // (likewise the counted wait of phase A: its unconditional loads and the parked index word double <3, GRAD>'s spills, so the
  // GRAD instances keep conditional loads and the index check in a loop, and with them one wait for everything)
  constexpr bool EARLY = !GRAD;
  // (PAIR_GATHER -- both members' gathers ahead of either contraction, gather_pair -- keeps two products alive across a
  // contraction: taken by the three-table instances, where it costs neither scratch nor a wave per SIMD and is worth 2.6 % on the
  // default workload (LAB_NOTES R18); the one- and two-table instances would lose a workgroup per CU, the wider ones have no registers
  // left: profiles/r18a_lean_kernel_resources.txt)
  constexpr bool PAIR_GATHER = !GRAD && NL == 0 && NT == 3;
  // (LAB_NOTES R19: instructions off a bundle's serial path, each taken where PAIR_GATHER is -- the other instances keep the
  // parent's instructions.  STORE_BRANCH: the stored product under a scalar branch on its flag bit; ONE_VERDICT: rescale_kmax;
  // LDS_ADDR: the main loop's LDS accesses by integer byte address, the array's base folded into the lane's offsets once)
  constexpr bool STORE_BRANCH = PAIR_GATHER;
  constexpr bool ONE_VERDICT = PAIR_GATHER;
  constexpr bool LDS_ADDR = PAIR_GATHER;
  // (LAB_NOTES R20: the wave reductions outside the main loop on PACKED vectors -- a lane holds 4 (PACKED_NORM) or 2 (PACKED_HOIST)
  // consecutive entries, the lowest levels of wave_sum's tree are in-lane adds, and the cross-lane levels serve four slots, or two
  // rows, at once.  wave_sum IS the balanced pairwise tree over entries 0..63 in index order, so the totals have its bits.  Taken
  // where PAIR_GATHER is, X = 64 only: PADX rows are shorter than a wave, GRAD keeps gst per row; the MULTI instance spills 20
  // bytes with PACKED_HOIST and takes the tail alone: profiles/r20a_lean_kernel_resources.txt)
  constexpr bool PACKED_NORM = PAIR_GATHER && !PADX;
  constexpr bool PACKED_HOIST = PAIR_GATHER && !PADX && !MULTI;
  static_assert(!(GRAD && PADX), "the GRAD form of phase A loads whole rows: X = 64 only");

  LaneGeo G;
  const int c_ = (lane & 7) | ((lane >> 1) & 8), b3_ = (lane >> 3) & 1, R_ = 4 * wave + (b3_ | ((lane >> 5) << 1));
  {
    const int b5 = lane >> 5, b4 = (lane >> 4) & 1, b2 = (lane >> 2) & 1;
    G.tm0 = (32 * b3_ + 2 * c_) * 8;
    G.tm1 = (32 * (1 - b3_) + 2 * c_) * 8;
    G.mt = 4 * R_ * 8;
    G.red_tm = (4 * R_ + 2 * b4 + b2) * 8;
    G.red_mt = (wave * 64 + 32 * b3_ + 2 * c_ + b5) * 8;
    G.up = b2 != 0;
    G.st_tm = wave == 0 && (lane & 0x28) == 0;
    G.st_mt = (lane & 0x17) == 0;
    G.wr_tm = (lane & 3) == 0;
    if (LDS_ADDR) { const int base = lds_addr(work); G.tm0 += base; G.tm1 += base; G.mt += base; }     // gather_pair's only
  }
  const int lane8 = LDS_ADDR ? lds_addr(work) + lane * 8 : 0;       // LDS_ADDR: the address of entry `lane` of message slot 0

  if (t == 0) f.bail[g] = 0;
  int g_kind = 0, g_obs = 0, g_lab = 0;           // GRAD: unary factor t's kind / observed column / label, parked until the
  if (GRAD && t < d.U) {                          // unary rows have landed (the loads retire in order ahead of them)
    g_kind = gf.unary_kind[t]; g_obs = gf.unary_obs[(size_t)g * d.U + t]; g_lab = gf.unary_label[(size_t)g * d.U + t];
  }
  // ---- phase A: every HBM load of the graph is issued before anything waits: unary rows first (they are needed
  //      first and vmcnt retires in order), then the tables, then the (dense) index check and the micro-op image.
  //      Every load after the rows is issued unconditionally -- one that has nothing to fetch reads the head of the
  //      micro-op image (padded to 2 KB by build_lean_program) and its value is never looked at -- so that the number
  //      of loads behind the rows is the same on every path and the wait for the rows is a counted one: the fill, the
  //      hoisted unary messages, the first vote and the constant products run while the tables are still arriving ----
  bool ok = true;
  const double* nowhere = reinterpret_cast<const double*>(f.image);
  constexpr int HB = 8;                       // unary rows per wave held in registers; more go round again below
  double ur[HB];
  int uslot[HB], ufac[HB];
  // PACKED_HOIST: two rows per wave instruction -- the lower half-wave row 2p, the upper one row 2p + 1, lane h of a half the
  // entries 2h and 2h + 1 (an empty entry reads the first 512 bytes of the image)
  const double* urow[HB];
  double2 ur2[HB / 2];
  const bool upper = lane >= 32;
  const int h2 = 2 * (lane & 31);
  {
    const Words16 hl = sload16(img_hoist + wave * 2 * f.HL);      // this wave's (unary slot, message slot) pairs, -1 padded
#pragma unroll
    for (int j = 0; j < HB; ++j) {
      const int u = hl.w[2 * j];
      uslot[j] = hl.w[2 * j + 1];
      ufac[j] = u;
      if (PACKED_HOIST) {
        // (the index word and the range check as below; the row's address stays a scalar)
        int row = -1;
        if (u >= 0) row = f.dense ? g * d.U + u : as_const(d.unary_tab)[(size_t)g * d.U + u];
        const bool in = (unsigned)row < (unsigned)d.n_unary_tables;
        if (u >= 0 && !in) ok = false;
        urow[j] = in ? d.unary_tables + (size_t)row * 64 : nowhere;
      } else if (EARLY) {
        // the index word of an entry that exists only (a scalar load, outside the count; a graph without unary factors brings
        // no unary_tab); an empty entry or a row out of range loads a value nobody uses -- uslot < 0 skips it, !ok skips the
        // graph; PADX lanes past X are zeroed where the row is used
        int row = -1;
        if (u >= 0) row = f.dense ? g * d.U + u : as_const(d.unary_tab)[(size_t)g * d.U + u];
        const bool in = (unsigned)row < (unsigned)d.n_unary_tables;
        if (u >= 0 && !in) ok = false;
        const double* at = in ? d.unary_tables + (size_t)row * X + (PADX ? min(lane, X - 1) : lane) : nowhere;
        ur[j] = *at;
      } else {
        ur[j] = 0.0;
        if (u >= 0) {
          const int row = f.dense ? g * d.U + u : as_const(d.unary_tab)[(size_t)g * d.U + u];
          if ((unsigned)row >= (unsigned)d.n_unary_tables) ok = false;
          else ur[j] = d.unary_tables[(size_t)row * X + lane];
        }
      }
    }
    if (PACKED_HOIST) {
#pragma unroll
      for (int p = 0; p < HB / 2; ++p) ur2[p] = *reinterpret_cast<const double2*>((upper ? urow[2 * p + 1] : urow[2 * p]) + h2);
    }
  }
  double2 tab[NT][4][2];
#pragma unroll
  for (int p = 0; p < NT; ++p) {
    if (!PADX && EARLY) {
      const int pc = p < d.P ? p : 0;
      const int ti = f.dense ? g * d.P + pc : as_const(d.pair_tab)[(size_t)g * d.P + pc];
      const bool in = (unsigned)ti < (unsigned)d.n_pair_tables;
      if (p < d.P && !in) ok = false;
      const double* T = (p < d.P && in) ? d.pair_tables + (size_t)ti * 4096 + (size_t)(4 * R_) * 64 + 2 * c_ : nowhere;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        tab[p][r][0] = NT_LOAD2(T + r * 64 + 32 * b3_);
        tab[p][r][1] = NT_LOAD2(T + r * 64 + 32 * (1 - b3_));
      }
    } else if (p < d.P) {
      const int ti = f.dense ? g * d.P + p : as_const(d.pair_tab)[(size_t)g * d.P + p];
      if ((unsigned)ti >= (unsigned)d.n_pair_tables) { ok = false; continue; }
      if (!PADX) {
        const double* T = d.pair_tables + (size_t)ti * 4096 + (size_t)(4 * R_) * 64 + 2 * c_;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          tab[p][r][0] = NT_LOAD2(T + r * 64 + 32 * b3_);
          tab[p][r][1] = NT_LOAD2(T + r * 64 + 32 * (1 - b3_));
        }
      } else {
        const double* T = d.pair_tables + (size_t)ti * X * X;
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int row = 4 * R_ + r, col = 32 * (k ? 1 - b3_ : b3_) + 2 * c_;
            tab[p][r][k].x = (row < X && col < X) ? T[(size_t)row * X + col] : 0.0;
            tab[p][r][k].y = (row < X && col + 1 < X) ? T[(size_t)row * X + col + 1] : 0.0;
          }
      }
    }
  }
  // tables NT .. NT+NL-1: straight into LDS (LDS-DMA: no registers; lane l of a wave-instruction lands at base + 16 l, which
  // is exactly the [r * 2 + k][thread] image), waited for with the register tables before the sweeps start
#pragma unroll
  for (int p = NT; p < NT + NL; ++p) {
    if (p < d.P && !PADX) {
      const int ti = f.dense ? g * d.P + p : as_const(d.pair_tab)[(size_t)g * d.P + p];
      if ((unsigned)ti >= (unsigned)d.n_pair_tables) { ok = false; continue; }
      const double* T = d.pair_tables + (size_t)ti * 4096 + (size_t)(4 * R_) * 64 + 2 * c_;
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          typedef __attribute__((address_space(3))) void* lds_ptr;
          typedef const __attribute__((address_space(1))) void* glb_ptr;
          double2* dst = tl + ((p - NT) * 8 + r * 2 + k) * WG + wave * 64;          // wave-uniform
          __builtin_amdgcn_global_load_lds((glb_ptr)(T + r * 64 + 32 * (k ? 1 - b3_ : b3_)), (lds_ptr)dst, 16, 0, 0);
        }
    }
  }
  // MLBP_SWEEP_DENSE_TABLES is a statement about the index arrays; it is checked off the critical path: thread i < P + U
  // (lean_plan keeps P + U within the workgroup) requests word i behind the tables, parks it in a register and compares it
  // after the sweeps: a false statement sends the graph to the exact kernel, which reads the arrays.
  int dense_word = 0;
  bool dense_ok = true;
  if (EARLY) {
    const int i = min(t, d.P + d.U - 1);
    const int32_t* at = i < d.P ? d.pair_tab + (size_t)g * d.P + i : d.unary_tab + (size_t)g * d.U + (i - d.P);
    dense_word = *(f.dense ? at : f.image);
  } else if (f.dense) {
    for (int i = t; i < d.P + d.U; i += WG)
      dense_ok &= i < d.P ? d.pair_tab[(size_t)g * d.P + i] == g * d.P + i : d.unary_tab[(size_t)g * d.U + (i - d.P)] == g * d.U + (i - d.P);
  }
  // the micro-op image, requested behind the tables (it is first read when the sweeps start, i.e. when the tables are
  // there) and parked in registers until then
  constexpr int PW = 2;
  int32_t pre[PW];
#pragma unroll
  for (int q = 0; q < (STATIC ? 0 : PW); ++q)
    pre[q] = EARLY ? f.image[min(t + q * WG, 16 * (f.n_bundles + 1) - 1)] : ((t + q * WG < 16 * (f.n_bundles + 1)) ? f.image[t + q * WG] : 0);
  unsigned bad_key = 0;
  {
    double2* dst = reinterpret_cast<double2*>(work);
    const int x0 = (2 * t) & 63;                                  // states of the double2 this thread writes (stride 256 keeps them)
    const double2 uni2 = PADX ? make_double2(x0 < X ? uniform : 0.0, x0 + 1 < X ? uniform : 0.0) : make_double2(uniform, uniform);
    if (f.init) {
      for (int i = t; i < d.n_msgs * 32; i += WG) dst[i] = uni2;
    } else if (!PADX) {
      const double2* src = reinterpret_cast<const double2*>(gm);
      for (int i = t; i < d.n_msgs * 32; i += WG) {
        const double2 v = src[i];
        bad_key = max(bad_key, max(mag_key(v.x), mag_key(v.y)));
        dst[i] = v;
      }
    } else {
      for (int i = t; i < d.n_msgs * 64; i += WG) {
        const int slot = i >> 6, x = i & 63;
        const double v = x < X ? gm[(size_t)slot * X + x] : 0.0;
        bad_key = max(bad_key, mag_key(v));
        work[i] = v;
      }
    }
    if (t < 32) dst[d.n_msgs * 32 + t] = uni2;                                           // ext slot 0: the uniform vector
    if (t >= 32 && t < 64) dst[(d.n_msgs + f.n_ext - 1) * 32 + (t - 32)] = make_double2(1.0, 1.0);   // last ext slot: ones
  }
  lds_barrier();        // the fill above and the unary messages below write the same slots from different waves
  // hoisted unary messages (exact values: they are outputs); further rounds only when a wave has more than HB rows.  A row
  // whose total is not positive (all zero, or NaN) flags its graph like a zero-total update inside the sweeps (rescale): the
  // zero-sum -> uniform rule of LBP.py:655-657 acts, and every graph it acts on goes to the exact kernel -- one rule for the
  // prologue and the main loop, and exact_count counts all such graphs
  if (PACKED_HOIST) {
    // two rows a pass.  Level 1 of the tree is the in-lane add, levels 2-5 the DPP steps (a half-wave's 32 lanes then hold
    // R0 + R1 in their first row of 16 and R2 + R3 in their second, R = a sum of 16 consecutive entries), level 6 adds the two.
    // The quotient, the verdict and the store all stay in this layout
#pragma unroll
    for (int p = 0; p < HB / 2; ++p) {
      if (uslot[2 * p] >= 0 || uslot[2 * p + 1] >= 0) {
        const int slot = upper ? uslot[2 * p + 1] : uslot[2 * p];
        const double2 r = ur2[p];
        const double q = row16_sum(r.x + r.y);
        const double s = swapadd16(q, q);
        const double2 m = make_double2(renorm(r.x, s, uniform, true), renorm(r.y, s, uniform, true));
        if (slot >= 0) {
          bad_key = max(bad_key, s > 0.0 ? max(mag_key(m.x), mag_key(m.y)) : KEY_BAD);
          *reinterpret_cast<double2*>(work + slot * 64 + h2) = m;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < (PACKED_HOIST ? 0 : HB); ++j) {
    if (uslot[j] >= 0) {
      const double r = (!PADX || lane < X) ? ur[j] : 0.0;
      const double s = wave_sum(r);
      const double m = renorm(r, s, uni_l, true);
      bad_key = max(bad_key, s > 0.0 ? mag_key(m) : KEY_BAD);
      work[uslot[j] * 64 + lane] = m;
      if (GRAD && lane == 0) { gst[ufac[j]] = uslot[j]; gst[d.U + ufac[j]] = s > 0.0 ? 1 : 0; }
    }
  }
  if (GRAD && t < d.U) { gst[2 * d.U + t] = g_kind; gst[3 * d.U + t] = g_obs; gst[4 * d.U + t] = g_lab; }
  for (int j = HB; j < f.HL; ++j) {
    const const_i32p hp = as_const(img_hoist + (wave * f.HL + j) * 2);
    const int u = hp[0], slot = hp[1];
    if (u < 0) break;
    const int row = f.dense ? g * d.U + u : as_const(d.unary_tab)[(size_t)g * d.U + u];
    double r = 0.0;
    if ((unsigned)row >= (unsigned)d.n_unary_tables) ok = false;
    else if (!PADX || lane < X) r = d.unary_tables[(size_t)row * X + lane];
    const double s = wave_sum(r);
    const double m = renorm(r, s, uni_l, true);
    bad_key = max(bad_key, s > 0.0 ? mag_key(m) : KEY_BAD);
    work[slot * 64 + lane] = m;
    if (GRAD && lane == 0) { gst[u] = slot; gst[d.U + u] = s > 0.0 ? 1 : 0; }
  }
  if (LEAN_SYNC ? vote_any(!ok, votes, wave, lane) : !__syncthreads_and(ok ? 1 : 0)) {       // an out-of-range table index: skip the graph, raise the status word
    if (t == 0) atomicExch(d.status, 1);
    // "skipped" means untouched -- except that a call which was asked to initialise leaves the graph initialised
    // (FactorGraph.initialize, LBP.py:211-216), not holding whatever the caller's buffer held
    if (f.init)
      for (int i = t; i < d.n_msgs * X; i += WG) gm[i] = uniform;
    return;
  }
  // constant products: uniform x the hoisted messages a variable multiplies in, in facset order (LBP.py:381-386);
  // lists are 16 words (count, 15 slots padded with the all-ones slot), wave k & 3 takes list k
  for (int k = wave; k < f.n_cprod; k += 4) {
    const Words16 cl = sload16(img_cprod + 16 * k);
    double acc = uni_l;
#pragma unroll
    for (int q0 = 1; q0 < 16; q0 += 5) {
      if (cl.w[0] >= q0) {
        double m[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) m[q] = work[cl.w[q0 + q] * 64 + lane];
#pragma unroll
        for (int q = 0; q < 5; ++q) acc *= m[q];
      }
    }
    bad_key = max(bad_key, mag_key(acc));               // a non-finite intermediate stays non-finite: nan_to_num territory
    work[(d.n_msgs + 1 + k) * 64 + lane] = acc;
  }
  // the micro-ops go into LDS ahead of the prologue's verdict: the vote's barrier publishes them, and the LDS-DMA tables that
  // have landed, for the main loop (a barrier of their own cost what a bundle's does)
  auto fill_limg = [&]() {
    if (NL > 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
    for (int q = 0; q < PW; ++q)
      if (t + q * WG < 16 * (f.n_bundles + 1)) limg[t + q * WG] = pre[q];
    for (int i = t + PW * WG; i < 16 * (f.n_bundles + 1); i += WG) limg[i] = f.image[i];
  };
  if (LEAN_SYNC && !STATIC) fill_limg();
  if (LEAN_SYNC ? vote_any(bad_key >= KEY_BAD, votes + 1024, wave, lane) : __syncthreads_or(bad_key >= KEY_BAD ? 1 : 0) != 0) {
    if (t == 0) f.bail[g] = 1;                    // bail codes: 1 prologue, 2 main loop, 3 final pass
    return;
  }
  if (!LEAN_SYNC) { fill_limg(); lds_barrier(); }

  // ---- main loop: identical in all four waves; one barrier per bundle.  The micro-ops sit in LDS; a bundle's 16 words
  //      are read (broadcast) one bundle ahead ----
  char* wb = reinterpret_cast<char*>(work);
  int parity = 0, bad = 0;
  unsigned kmax = 0, some = ~0u;               // ONE_VERDICT (rescale_kmax)
  double carry = 1.0;
  const int4* li = reinterpret_cast<const int4*>(limg);
  if constexpr (STATIC) {
#ifdef MLBP_LEAN_STATIC
    static_assert(PAIR_GATHER && NT == 3, "the static main loop is the PAIR_GATHER instance's");
    const StaticCtx c = {wb, reinterpret_cast<char*>(red), G, lane8, lane};
    StaticBundle<0>::run(c, tab, some, kmax);
#endif
  } else {
  int4 A0 = li[0], A1 = li[1], B0 = li[2], B1 = li[3];
  for (int k = 0; k < f.n_bundles; ++k) {
    // the image is padded by one bundle.  (PAIR_GATHER asks for the next words behind its gathers: ahead of them, sixteen more
    // registers are alive where the bundle's pressure peaks, and the third table spills)
    int4 nA0, nA1, nB0, nB1;
#define MLBP_FETCH_NEXT() (nA0 = li[4 * k + 4], nA1 = li[4 * k + 5], nB0 = li[4 * k + 6], nB1 = li[4 * k + 7])
    if (!PAIR_GATHER) MLBP_FETCH_NEXT();
    const int fA = __builtin_amdgcn_readfirstlane(A0.x), fB = __builtin_amdgcn_readfirstlane(B0.x);
    if (fA & UOP_VAR) {
      if (PAIR_GATHER) MLBP_FETCH_NEXT();
      // a lone variable update: the product, lane = state, the same in every wave; no contraction, no barrier
      // a product of more than four sources is a chain of links; the running product stays in a register between
      // them and only the last link stores (every wave stores the same value once: no read-modify-write of a slot
      // that another wave may still be writing)
      const int nsrc = (fA >> UOP_NSRC_SHIFT) & 15;
      double m = LDS_ADDR ? lds1_at(A0.y + lane8) : work[(A0.y >> 3) + lane];
      const double m2 = LDS_ADDR ? lds1_at(A0.z + lane8) : work[(A0.z >> 3) + lane];          // (padded with the all-ones slot, like a contraction's list)
      if (fA & UOP_CARRY_IN) m *= carry;
      m *= m2;
      if (nsrc > 2) {
        const double m3 = LDS_ADDR ? lds1_at(A0.w + lane8) : work[(A0.w >> 3) + lane];
        const double m4 = LDS_ADDR ? lds1_at(A1.x + lane8) : work[(A1.x >> 3) + lane];
        m *= m3;
        m *= m4;
      }
      if (fA & UOP_CARRY_OUT) carry = m;
      else if (LDS_ADDR) lds1_put(A1.y + lane8, m);
      else work[(A1.y >> 3) + lane] = m;
    } else {
      char* redP = reinterpret_cast<char*>(red) + parity * 4096;
      const bool two = !(fB & UOP_NOP);
      if (PAIR_GATHER) {
        Src mA, mB;
        gather_pair<STORE_BRANCH, LDS_ADDR>(wb, fA, A0, A1, fB, B0, B1, G, mA, mB);
        MLBP_FETCH_NEXT();
        front_gathered<NT>(tab, fA, mA, G, redP);
        if (two) front_gathered<NT>(tab, fB, mB, G, redP + 2048);
      } else {
        front<NT, NL>(tab, tl + t, wb, fA, A0, A1, G, redP);
        if (two) front<NT, NL>(tab, tl + t, wb, fB, B0, B1, G, redP + 2048);
      }
      lds_barrier();
      const double* rd = reinterpret_cast<const double*>(redP);
      double rA = rd[lane];
      if (fA & UOP_MT) rA = (rA + rd[64 + lane]) + (rd[128 + lane] + rd[192 + lane]);
      if (LDS_ADDR) lds1_put(A1.z + lane8, ONE_VERDICT ? rescale_kmax(rA, some, kmax) : rescale(rA, bad));
      else work[(A1.z >> 3) + lane] = ONE_VERDICT ? rescale_kmax(rA, some, kmax) : rescale(rA, bad);
      if (two) {
        double rB = rd[256 + lane];
        if (fB & UOP_MT) rB = (rB + rd[320 + lane]) + (rd[384 + lane] + rd[448 + lane]);
        if (LDS_ADDR) lds1_put(B1.z + lane8, ONE_VERDICT ? rescale_kmax(rB, some, kmax) : rescale(rB, bad));
        else work[(B1.z >> 3) + lane] = ONE_VERDICT ? rescale_kmax(rB, some, kmax) : rescale(rB, bad);
      }
      parity ^= 1;
    }
    A0 = nA0; A1 = nA1; B0 = nB0; B1 = nB1;
#undef MLBP_FETCH_NEXT
  }
  }
  if (ONE_VERDICT) bad = some == 0 || __ballot(kmax >= KEY_BAD) != 0;
  if (bad) {                                      // the same in every wave: the inputs were identical
    if (t == 0) f.bail[g] = 2;
    return;
  }
  lds_barrier();
  // ---- read-out (VariableNode.get_marginal, LBP.py:392-400) straight from the scaled messages: the marginal is
  //      normalised, so the scales cancel; constant part = the variable's constant product ----
  double marg[2] = {0.0, 0.0};
  if (EARLY) dense_ok = !f.dense || t >= d.P + d.U || dense_word == (t < d.P ? g * d.P + t : g * d.U + (t - d.P));
  bool bad_out = !dense_ok;
  // PACKED_NORM: the first four words of the wave's written-slot list (16-byte aligned: every part of the image is a multiple of
  // four words, WL too), one scalar load that lands while the read-out runs
  v4i wq = {0, 0, 0, 0};
  if (PACKED_NORM) wq = sload4(img_written + wave * f.WL);
  if (f.readout) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = wave + 4 * j;
      if (v < d.n_vars) {
        const Words16 rl = sload16(f.readout + 16 * v);
        double acc = work[rl.w[1] * 64 + lane];
#pragma unroll
        for (int q0 = 2; q0 < 16; q0 += 7) {
          if (rl.w[0] >= q0) {
            double m[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) m[q] = work[rl.w[q0 + q] * 64 + lane];
#pragma unroll
            for (int q = 0; q < 7; ++q) acc *= m[q];
          }
        }
        const unsigned key = wave_max_u32(mag_key(acc));
        bad_out |= key >= KEY_BAD || key < KEY_MIN;
        marg[j] = acc / wave_sum(acc);
      }
    }
    for (int v = wave + 8; v < d.n_vars; v += 4) {       // graphs with more than 8 variables: one at a time
      const Words16 rl = sload16(f.readout + 16 * v);
      double acc = work[rl.w[1] * 64 + lane];
      for (int q = 2; q <= rl.w[0]; ++q) acc *= work[as_const(f.readout + 16 * v)[q] * 64 + lane];
      const unsigned key = wave_max_u32(mag_key(acc));
      bad_out |= key >= KEY_BAD || key < KEY_MIN;
      if (!bad_out) d.marginals[((size_t)g * d.n_vars + v) * 64 + lane] = acc / wave_sum(acc);   // (redone by the exact kernel when flagged)
    }
  }
  lds_barrier();        // the normalisation below rewrites slots the read-out above has just read
  // ---- the deferred normalisations (only when the messages go back to memory): exactly the slots the program wrote,
  //      wave w takes its WL-entry list, four at a time ----
  if (f.keep || GRAD) {      // (GRAD: the same validity check guards the messages the gradient reads)
    // PACKED_NORM: the four slots of a pass in one reduction -- lane group s = lane >> 4 takes the s-th listed slot, its lane c
    // the entries 4c .. 4c + 3.  Levels 1-2 of the tree are in-lane adds, levels 3-6 the four DPP steps inside the group
    for (int j0 = 0; PACKED_NORM && j0 < f.WL; j0 += 4) {
      const v4i w = wq;                                             // (asked for a pass ahead: the first one ahead of the read-out)
      if (j0 + 4 < f.WL) wq = sload4(img_written + wave * f.WL + j0 + 4);
      const int slot = upper ? ((lane & 16) ? w.w : w.z) : ((lane & 16) ? w.y : w.x);
      const int at = slot * 512 + (lane & 15) * 32;
      double2 a = make_double2(1.0, 1.0), b = a;                    // (a padding entry: ones, nothing stored)
      if (slot >= 0) { a = lds2(wb + at); b = lds2(wb + at + 16); }
      const unsigned key = row16_max_u32(max(max(mag_key(a.x), mag_key(a.y)), max(mag_key(b.x), mag_key(b.y))));
      bad_out |= key >= KEY_BAD || key < KEY_MIN;         // a variable product underflowed or vanished
      const double s = row16_sum((a.x + a.y) + (b.x + b.y));
      if (slot >= 0) {
        *reinterpret_cast<double2*>(wb + at) = make_double2(a.x / s, a.y / s);
        *reinterpret_cast<double2*>(wb + at + 16) = make_double2(b.x / s, b.y / s);
      }
    }
    for (int j0 = 0; !PACKED_NORM && j0 < f.WL; j0 += 4) {
      const const_i32p wl = as_const(img_written + wave * f.WL + j0);
      int slot[4];
      double v[4], s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) { slot[j] = wl[j]; v[j] = slot[j] >= 0 ? work[slot[j] * 64 + lane] : 1.0; }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned key = wave_max_u32(mag_key(v[j]));
        bad_out |= key >= KEY_BAD || key < KEY_MIN;       // a variable product underflowed or vanished
        s[j] = wave_sum(v[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (slot[j] >= 0) work[slot[j] * 64 + lane] = v[j] / s[j];
    }
  }
  if (LEAN_SYNC ? vote_any(bad_out, votes, wave, lane) : __syncthreads_or(bad_out ? 1 : 0) != 0) {         // nothing of a flagged graph is written back
    if (t == 0) f.bail[g] = 3;
    return;
  }
  if (f.keep && !PADX) {
    const double2* src = reinterpret_cast<const double2*>(work);
    double2* dst = reinterpret_cast<double2*>(gm);
    for (int i = t; i < d.n_msgs * 32; i += WG) NT_STORE2(dst + i, src[i]);
  } else if (f.keep) {
    for (int i = t; i < d.n_msgs * 64; i += WG)
      if ((i & 63) < X) gm[(size_t)(i >> 6) * X + (i & 63)] = work[i];
  }
  if (f.readout) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int v = wave + 4 * j;
      if (v < d.n_vars) __builtin_nontemporal_store(marg[j], &d.marginals[((size_t)g * d.n_vars + v) * 64 + lane]);
    }
  }
  if (GRAD) {                 // (the verdict barrier above has published the final normalisation)
    gradient_epilogue<NT>(d, gf, tab, reinterpret_cast<const char*>(work), gst, reinterpret_cast<double*>(red), G, g, R_, c_, b3_);
  }
}

}  // namespace

#endif
