// qpd_mop.hpp -- the fast engine's plan vocabulary: the micro-op record the
// plan compiler (qpd_plan.hpp, host code) writes and the kernels (qpd_fast.hip)
// interpret.  No HIP: the plan compiler's CPU test builds it with g++.
#pragma once
#include <stdint.h>

#include "qpd_fast_switches.hpp"
#include "qpd_types.hpp"

namespace qpd {

constexpr int OP_BOT3 = 9;    // fused bottom subtree of height 3 (fast engine only)
constexpr int OP_IMPORT = 10; // frozen-prefix stages (see lut_prefix_kernel): rows / metric from a stage's records, or zeros
constexpr int OP_EXPORT = 11; // lut_prefix_kernel only: live rows into the stage's records (FastPlan::pfx)

enum MopFlag : int32_t {
    MF_SRC_LDS = 1,   // S[d] in LDS
    MF_DST_LDS = 2,   // destination rows in LDS
    MF_U_LDS = 4,     // U rows read by the op in LDS
    MF_TO_R = 8,      // finished node is a right child (or the root): write R, not U
    MF_SYNC = 16,     // drain the global slab before this op (see place_syncs)
    MF_R_LDS = 32,    // R rows read by the op (COMB) in LDS
    MF_CHAN = 64,     // S[d] is the channel input (d == 0)
    MF_R1_LDS = 128,  // R1 (> 16 elements): argsort in the free LDS tail starting at row u_row
    MF_PRE = 256,     // S[1] of the root's left child / the root g inputs: words of the frame's
                      // pre-pass row (root_pre_kernel), read without a slot pointer
    MF_GSEL = 512,    // root g in pre-mode: nibble select between g(y, 0) and g(y, 1) by u
    MF_BFG = 1024,    // BOT3 whose 8 input symbols are f (or g, MF_BG) of its depth n-4 parent's 16:
    MF_BG = 2048,     //   the parent's F / G op folded in (src = S[n-4], table at tab2, U[n-3] at u_row)
    MF_BCOMB = 4096,  // right BOT3 that also runs its parent's combine (dst = U/R[n-4])
    MF_VUNI = 8192,   // special node whose elements share one quanta row (v <= 16): quanta and
                      //   R1 ranks are looked up in a register row instead of gathered per element
    MF_ZERO = 16384,  // OP_IMPORT: zero rows (partial sums of the frozen prefix) instead of record words
    MF_PM = 32768,    // OP_IMPORT: the path metric (a double in words src_row, src_row + 1 of the record)
    MF_VIA_PS = 65536,   // OP_EXPORT: the row is read through the path's S pointer of depth sh_src / 4
    MF_VIA_PU = 131072,  //   ... or its U pointer (else the lane's own row: R rows)
    MF_XBUF = 262144,    // OP_IMPORT: from a prefix stage's records (address and layout in the op record)
    MF_FF = 524288,      // F / G (SCL-LUT) that also runs the f of its left child at depth d+1 from
                         //   the words it just computed (fuse_descent): S[d+2] at r_row, the
                         //   child's table at tab2, its S pointer field at pad1
    MF_FF_DL = 1048576,  //   ... S[d+2] in LDS
    MF_BC2 = 2097152,    // right BOT3 with MF_BCOMB and MF_TO_R that also runs the combine of its
                         //   grandparent at depth n-5 (fold_combine): U[n-4] of the left sibling at
                         //   r_row (pointer field pad1 & 255), result to row pad1 >> 16 (its U
                         //   pointer field (pad1 >> 8) & 255) instead of R[n-4] at dst_row
    MF_BC2_ULDS = 4194304,  //   ... that U row in LDS
    MF_BC2_DLDS = 8388608,  //   ... the result row in LDS
    MF_BC2_TOR = 16777216,  //   ... the grandparent is a right child (R row: no pointer update)
    MF_BOTX = 33554432,     // BOT3 of a subtree with FastSCL special nodes of size 4 / 2 (botx_op)
    MF_R1_RK = 67108864,    // R1 with one quanta row: symbol s's rank in bits 4s..4s+3 of r_row | tab2 << 32 and
                            //   its sign in bit s of pad1 (r1_prep: no per-element rank lookups)
    MF_SFG = 134217728,     // size-8 special node (FastSCL-LUT, L = 8) that computes its 8 symbols as f of its
                            //   depth n-4 parent's 16 (src = S[n-4], the parent's table at tab): no F op
    MF_SGG = 268435456,     //   ... as g of them, u = the left sibling's U[n-3] at u_row (sh_u): no G op
    MF_SCOMB = 536870912,   //   ... and runs the parent's combine with that U[n-3] (dst = the parent's): no COMB
    MF_LO = 1073741824,     // F / G / BOT3 of a plan whose S rows of >= 8 symbols are in lookup order
                            //   (QPD_ROW_BYTEIDX, FastHostPlan::row_lo): the op's source (a row or pre-pass row of
                            //   >= 8 symbols) is read, its destination (>= 8 symbols) written in that order
};

struct MOp {
    int32_t type, flags, d, node;
    int32_t cnt;      // F/G/COMB: ctemp = N>>(d+1); special: temp = N>>d; LEAF: frozen; BOT3: frozen mask
    int32_t src_row;  // S[d]
    int32_t dst_row;  // F/G: S[d+1]; COMB/special/BOT3: U[d] or R[d]; LEAF_L: U[n]; LEAF_R: R[n]
    int32_t u_row;    // G/COMB: U[d+1]; LEAF_R: U[n]
    int32_t r_row;    // COMB: R[d+1]; F/G with MF_FF: S[d+2]
    int32_t sh_src;   // 4*d: ps field of S[d]
    int32_t sh_u;     // G/COMB: 4*(d+1); LEAF_R: 4*n (depth 16: nibble 0, u_field in qpd_plan.hpp)
    int32_t sh_dst;   // F/G: 4*(d+1) (ps); COMB/special/BOT3 left child: 4*d (pu); LEAF_L: 4*n (pu)
    int32_t tab;      // F/LEAF_L: posi*32; G/LEAF_R: posi*64; BOT3: posi of the subtree root; R1: r1_rank offset
    int32_t vrow;     // LEAF: ((n-1)*N + k)*v; special: (d-1)*N + temp*node; BOT3: ((n-1)*N + 8*node)*v
    int32_t tab2;     // MF_BFG: the parent's table (f: posi*32, g: posi*64); MF_FF: the child's f table
    int32_t pad1;     // MF_FF: the child's S pointer field (4*(d+2))
};

constexpr int kSelInts = 128;  // per set: 64 slots + 64 junk slots (select_survivors8): two rows after the set's

// QPD_LEAF_T = 1 -- the depth n-1 tables are stored transposed (entry
// u * 256 + b * 16 + a: pack_tables in qpd_plan.hpp, leaf_idx in qpd_fast_bot.hpp).
#ifndef QPD_LEAF_T
#define QPD_LEAF_T 1
#endif

}  // namespace qpd
