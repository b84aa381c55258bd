// Compile-time tuning knobs of the gfx950 kernels, in one place.  Each default is the measured optimum
// of a same-box A/B (DESIGN.md sections 3-5, logs under profiles/); tools/build_obj_variants.sh builds a
// one-object library with any of them overridden (-DNAME=value) for such an A/B.
#pragma once

// ---- k_wino_om (wino.hip)
#ifndef WINO_OM_RING
#define WINO_OM_RING 2     // k_wino_om B-operand blocks in flight (4: 158 -> 170-177 us, r02_wino_om_ring_ab.log)
#endif

// ---- k_dcn (dcn.hip): the DCN core of the two-kernel path and of the _ext drop-in (dcn_v2.hip) at the STIF shape
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

// ---- k_dec1 / k_dec2 / k_dec2q (decoder.hip): no knobs.  What earlier A/Bs settled is fixed in the source, with its
// numbers at the line that fixes it: k_dec1's workgroups per CU (OCC1: 4, HR-image variants 3, MODE 2 2;
// r04_dec1_occ_ab.log, r04_dec1_occ4_ab.log), f16x3 stage 2 without an HR image by k_dec2q (r04_dec2q4_ab.log) in
// 8-wave workgroups with one layer-2 tile per weight segment (r06_dec_ab.log), the raw hardware sine (r05_sin_raw.log)
