// Compile-time tuning knobs of the gfx950 kernels, in one place.  Each default is the measured optimum
// of a same-box A/B (DESIGN.md sections 3-5, logs under profiles/); tools/build_obj_variants.sh builds a
// one-object library with any of them overridden (-DNAME=value) for such an A/B.
#pragma once

// ---- k_wino_om (wino.hip)
#ifndef WINO_OM_RING
#define WINO_OM_RING 2     // k_wino_om B-operand blocks in flight (4: 158 -> 170-177 us, r02_wino_om_ring_ab.log)
#endif

// ---- k_dcn (dcn.hip): the DCN core of the two-kernel path and the _ext drop-in at the STIF shape
#ifndef DCN_TH
// waves per workgroup: 4 (8-row two-row tiles, two workgroups per CU whose barriers and memory waits
// overlap): C0 L1 DCN 240 -> 223 us against 8 (r02_dcn_th_ab.log)
#define DCN_TH 4
#endif
#ifndef DCN_M
// staged margin (px) around the 3x3 footprint; samples beyond it use the global-load fallback.
// C0 L1: margin 2 / 3 / 4 / 6 / 8 -> 248 / 250 / 257 / 266 / 289 us (r02_dcn_margin_ab.log)
#define DCN_M 2
#endif
#ifndef DCN_MR2_MIN
#define DCN_MR2_MIN 1024   // two-row kernel from this many workgroups (512 measured no faster)
#endif

// ---- k_dec1 / k_dec2 / k_dec2q (decoder.hip)
#ifndef DEC1_OCC
// k_dec1 (MODE 0 / 1) workgroups per CU: 4 (36 KB LDS, 128 registers, the flow projection gathered in four
// 8-load quarters), 3 (52 KB, 168, halves) or 2 (69 KB, 256).  C0 dec1 869 -> 758 us (2 -> 3,
// r04_dec1_occ_ab.log) -> 720 us (3 -> 4; C2 11.6 -> 11.1 ms, r04_dec1_occ4_ab.log); all bit-identical
#define DEC1_OCC 4
#endif
#ifndef DEC2_Q16
// stage 2 (f16x3, LR-projection inputs) by k_dec2q: 16 pixels per wave, four waves per SIMD (128 VGPRs);
// C2 stage 2 17.55-17.79 -> 17.32-17.34 ms (r04_dec2q4_ab.log).  0 = k_dec2 (also the fp32 and
// high-resolution-image stages)
#define DEC2_Q16 1
#endif
#ifndef DEC2Q_NW
// k_dec2q waves per workgroup: 8 (two 80-KB workgroups per CU, one layer-2 tile per streamed weight segment) or
// 16 (one 160-KB workgroup, two tiles per segment: +27 %, r06_dec_ab.log)
#define DEC2Q_NW 8
#endif
#ifndef DEC2Q_KTS
#define DEC2Q_KTS (DEC2Q_NW == 16 ? 2 : 1)   // layer-2 tiles per streamed weight segment
#endif
static_assert(DEC1_OCC >= 2 && DEC1_OCC <= 4, "DEC1_OCC: k_dec1 is laid out for 2, 3 or 4 workgroups per CU");
static_assert(DEC2_Q16 == 0 || DEC2_Q16 == 1, "DEC2_Q16: 0 (k_dec2) or 1 (k_dec2q)");
