// qpd_fast_switches.hpp -- every compile-time switch of the fast engine
// (qpd_fast.hip and the qpd_fast_*.hpp headers it is made of) with its default.
// Every fast-engine header includes this file first, so a switch is defined
// before any use; the build reads an undefined one as an error (-Werror=undef,
// build.py).  A switch is set with -D (tools/build_variant.sh), QPD_VEC_CHAIN
// also by a unit before its include.
//
// Switches defined elsewhere, shared with the generic engine, the host planner
// or the generator:
//   QPD_DYN             qpd_common.hpp: tasks from a device queue (0: static grid-stride)
//   QPD_SEL_OPAQUE      qpd_common.hpp: select_survivors8's lane terms derived behind the identity test
//   QPD_LANE_READ_SHFL  qpd_common.hpp (#ifdef): lane_read / shfld by HIP's __shfl
//   QPD_LEAF_T          qpd_mop.hpp: the depth n-1 tables stored transposed
//   QPD_DEFAULT_SETS    qpd_plan.hpp: frame sets per wave of the list kinds
//   QPD_SETS3, QPD_DIAG qpd_plan.hpp / qpd_k_scl.hip (#ifdef): the three-set SCL-LUT kernel; planner diagnostics
//   QPD_MC_PAIRS, QPD_MC_WPE  qpd_mc.hip: the Monte-Carlo generator's kernel shape
#pragma once

// ---------------------------------------------------------------------------
// Product tuning
// ---------------------------------------------------------------------------
// Tested with #ifdef, no value (keep_all8, qpd_fast_select.hpp):
//   QPD_HI_IDENT   a conservative identity test on the keys' high words first: measured -0.5 % on SCL-LUT (r04e): off
//   QPD_IDENT_MAX  the group maximum by a 3-step DPP reduction (round 3): 1.1 % slower (r04q): off

// Waves per SIMD the register allocation targets: 6 (80 VGPRs) for one
// frame set, 4 (128 VGPRs) for two (5 for SCL-LUT, below), 6 for FastSCL's one set too (its special
// ops spill ~136 B at 80 VGPRs, yet with the task queue 6 waves beat 5 by 4%)
// -- the measured optima on MI355X.
#ifndef QPD_WPE1
#define QPD_WPE1 6
#endif
#ifndef QPD_WPE_FSCL
#define QPD_WPE_FSCL 6
#endif
#ifndef QPD_WPE2
#define QPD_WPE2 4
#endif
// SCL-LUT's two-set decode kernel: 5 waves per SIMD (96 VGPRs) since its path
// state takes one pointer word (PW1) and its BOT3 stages its loads (r04h:
// 44.3 vs 41.7 M frames/s at 4 waves)
#ifndef QPD_WPE2_SCL
#define QPD_WPE2_SCL 5
#endif
// FastSCL-LUT's two-set kernel: 4 waves per SIMD (128 VGPRs): its special-node
// and mixed-subtree code cost the whole kernel's allocation at 96 (the SCL-LUT op
// list on the FastSCL-LUT instantiation: 32.7 M frames/s at 5 waves, 37.7 M at 4,
// against 45.2 M on the SCL-LUT one; FastSCL-LUT 31.7 -> 37.7 M)
#ifndef QPD_WPE2_FSCL
#define QPD_WPE2_FSCL 4
#endif
#ifndef QPD_WPE3
#define QPD_WPE3 3
#endif
#ifndef QPD_WPE_W16
#define QPD_WPE_W16 4  // SCL-LUT at 9 <= L <= 16 (W16): with the all-at-once swaps 5.27 M frames/s at L = 16
                       // vs 5.09 for one swap per round at 4 or 5 waves (r06o; the swaps at 5: 4.52, spills)
#endif

#ifndef QPD_LUT_PACK2
#define QPD_LUT_PACK2 1  // lut_lds: the 8 results combined as 16-bit pairs (see there)
#endif
#ifndef QPD_LUT_OPAQUE
#define QPD_LUT_OPAQUE 1  // lut_lds: the odd elements' word kept whole for the last shift-or (see there)
#endif
#ifndef QPD_LUT_OPAQUE_XY  // lut_lds: X, Y whole before the index extraction (-3 % static VALU; SCL-LUT +0.7 %,
#define QPD_LUT_OPAQUE_XY 1  // FastSCL-LUT +0.9 %, profiles/r06za_ab_lut_xy.txt)
#endif

#ifndef QPD_BOT3_LAZY
#define QPD_BOT3_LAZY 1  // bot3_op: each stage issues the loads of the next (the list kinds; +0.5 % SCL-LUT at 5 waves, r04h)
#endif
// QPD_BOT3_BYTEIDX: bot3_op keeps W3 and W2 in interleaved order and looks its 12
// internal symbols up by the bytes as they lie (lut_byte, qpd_fast_lookup.hpp)
// instead of six lut_vec index builds per subtree and set.  Static count and
// A/B: profiles/AB_RECORDS.md, `bot3_byteidx_ab.jsonl`.
#ifndef QPD_BOT3_BYTEIDX
#define QPD_BOT3_BYTEIDX 1
#endif
// QPD_ROW_BYTEIDX: the plain kinds (SC-LUT, SCL-LUT, CA-SCL-LUT; every set count,
// W16, the prefix kernels) keep every S row of M >= 8 symbols in lookup order --
// word w holds elements 4w .. 4w+3 in the high nibbles of its bytes and elements
// 4w + M/2 .. in the low ones (M = 8: BOT3's W3 order) -- so the bytes of a stored
// word are the table indices a * 16 + b of the f / g op below it as they lie:
// lut_lds / lut_vec build no index words, an unfolded BOT3 no nib_interleave8
// (DESIGN.md section 3.2).  The plan compiler marks such plans (MF_LO,
// FastHostPlan::row_lo) and the pre-pass producers follow it.  FastSCL-LUT and
// FastSC-LUT keep the element order whatever the value: their special nodes and
// BOTX read symbols by nibble position.  Static count and A/B:
// profiles/AB_RECORDS.md, `row_byteidx_ab.jsonl`.
#ifndef QPD_ROW_BYTEIDX
#define QPD_ROW_BYTEIDX 1
#endif
#ifndef QPD_SPEC_ROT
#define QPD_SPEC_ROT 1  // special ops: one code copy, the sets rotated through slot 0 (else unrolled)
#endif
// The speculative right-leaf lookup (bot_pair): +1.3 % at 4 waves per SIMD,
// -1 % at the 5 the SCL-LUT kernel runs now (its registers; r04g / r04j): off.
#ifndef QPD_SPEC_RIGHT
#define QPD_SPEC_RIGHT 0
#endif
// QPD_VEC_CHAIN: lut_vec joins its results by one v_lshl_or per element (the
// compiler otherwise shifts each and merges them with v_or3: +0.5 VALU per
// lookup).  On in the FastSCL-LUT units (+0.5 %), off for SCL-LUT (-0.25 %:
// the serial chain costs it latency), profiles/r06v_ab_vec_chain.txt.
#ifndef QPD_VEC_CHAIN
#define QPD_VEC_CHAIN 0
#endif
// Bank swizzle of the g table's u = 1 half (QPD_GSWZ, a multiple of 8): entry
// (1, i) sits at byte 256 + (i ^ QPD_GSWZ), so that the lookups of one path
// pair that differ only in u -- the common case: a frame's paths share their
// symbols and differ in their decisions -- fall on different LDS banks instead
// of two dwords of one bank (ds_read_u8 banking: (byte / 4) mod 32 per 32-lane
// half-wave).  Simulated on the bench workload (tools/bank_sim.py): the g
// lookups' conflict cycles 44 % -> 17 % with 72; measured (profiles/r06f_*):
// SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE 15.8 % -> 10.0 % (SCL-LUT), 17.6 % ->
// 11.1 % (FastSCL-LUT) -- but 3.3 % / 1.5 % slower: the swizzle's VALU (the
// index bytes XOR u_byte * M: 6 per word of 8 lookups; 4 for M = 8, still -2.3 %)
// costs more than the conflicts, VALU issue being the kernel's nearest ceiling
// (a what-if without any conflicts and no extra VALU: +3.5 %).  Off; stage_tab
// puts the u = 1 chunks at lane ^ QPD_GSWZ / 8 (gtab_dw).
#ifndef QPD_GSWZ
#define QPD_GSWZ 0
#endif
#ifndef QPD_SLAB_AUX
#define QPD_SLAB_AUX 0  // cache-policy bits of the slab's buffer ops (2 = nt)
#endif
#ifndef QPD_BX_PIPE
#define QPD_BX_PIPE 0  // BOTX slot operands loaded one slot ahead
#endif
#ifndef QPD_R1_UNROLL
#define QPD_R1_UNROLL 0  // R1 layers unrolled
#endif

// ---------------------------------------------------------------------------
// Timing experiments that give wrong results
// ---------------------------------------------------------------------------
// Tested with #ifdef:
//   QPD_EXP_IDENT  keep_all8 returns its value: every L = 8 selection the identity (1) / none (0)
//   QPD_BXE        bits: 1 bx_spec_multi skipped, 2 its R1 nodes skipped, 4 botx_op's leaf pairs skipped

// Timing experiments only (wrong results): 0 = every op reads node 0's
// tables / the slab drops every access.
#ifndef QPD_EXP_TABMUL
#define QPD_EXP_TABMUL 1
#endif
#ifndef QPD_EXP_SLABMUL
#define QPD_EXP_SLABMUL 1
#endif

#ifndef QPD_EXP_LUTMASK
#define QPD_EXP_LUTMASK 0xFFFF  // timing experiments only (wrong results): 0x7F keeps every byte-table
                                // lookup inside one 128-B LDS bank row (no bank conflicts)
#endif

#ifndef QPD_EXP_NO_BOTX
#define QPD_EXP_NO_BOTX 0  // register-allocation experiments: botx_op compiled out (MF_BOTX ops then wrong)
#endif
#ifndef QPD_EXP_FSCL
#define QPD_EXP_FSCL 0  // code-quality experiments (wrong results for those ops): 2 no special ops,
                        // 4 no R1, 8 no R1 LDS introsort, 16 no REP, 32 / 64 r1_multi above 16 elements without
                        // layers / with a fixed argsort, 128 old partition loop, 256 no special
                        // ops at all, 512 no multi-set R0/REP, 1024 no multi-set R1
#endif
#ifndef QPD_EXP_NO_LDSTAB
#define QPD_EXP_NO_LDSTAB 0  // A/B: the f / g lookups by ds_bpermute from the table register (no byte tables)
#endif

// ---------------------------------------------------------------------------
// Diagnosis (tested with #ifdef)
// ---------------------------------------------------------------------------
//   QPD_POISON        its value written to every LDS word and slab row of a wave at the start of each
//                     task: a read of a row no op of the task wrote shows up as a parity difference
//   QPD_STAMPS        wave cycles per op class (lane k of each wave accumulates class k; flushed into
//                     FastPlan::stamps once per task).  Class = 2*type + (op syncs), or
//   QPD_STAMPS_DEPTH  by depth
