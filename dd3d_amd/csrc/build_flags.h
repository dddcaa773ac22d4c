// Build-time knobs of libdd3d_hip.so: every -DDD3D_...=... a translation unit was compiled with, as a string.
//
// The product build (__graft_entry__.build()) passes none: dd3d_build_flags() then returns "" and dd3d_amd/hip.py loads the library.  A
// library built with any of them -- the variants of tests/tools/build_variant.sh; all of them compute CORRECT results, the knobs set
// LDS budgets, the stem kernel's shape and the row kernel's timing probe -- says so, and hip.py refuses it unless the caller selected it explicitly (DD3D_HIP_LIB /
// DD3D_ALLOW_VARIANT_LIB=1), so that a stray -D cannot ship as the product library unnoticed (round-4 verdict).  Timing experiments that
// compute WRONG results (ablations of the K loop, racy barriers) are not in these sources at all: tests/tools/variants/*.patch.
//
// Included by common.h BEFORE any translation unit gives a knob its default (`#ifndef X / #define X default`), so "defined here" means
// "given on the command line".
#pragma once
#define DD3D_BF_STR2(x) #x
#define DD3D_BF_STR(x) DD3D_BF_STR2(x)
#ifdef DD3D_LDS_KIB_4W
#define DD3D_BF_0 " DD3D_LDS_KIB_4W=" DD3D_BF_STR(DD3D_LDS_KIB_4W)
#else
#define DD3D_BF_0 ""
#endif
#ifdef DD3D_LDS_KIB_8W
#define DD3D_BF_1 " DD3D_LDS_KIB_8W=" DD3D_BF_STR(DD3D_LDS_KIB_8W)
#else
#define DD3D_BF_1 ""
#endif
#ifdef DD3D_ROW_LDS_KIB_4W
#define DD3D_BF_2 " DD3D_ROW_LDS_KIB_4W=" DD3D_BF_STR(DD3D_ROW_LDS_KIB_4W)
#else
#define DD3D_BF_2 ""
#endif
#ifdef DD3D_ROW_LDS_KIB_8W
#define DD3D_BF_3 " DD3D_ROW_LDS_KIB_8W=" DD3D_BF_STR(DD3D_ROW_LDS_KIB_8W)
#else
#define DD3D_BF_3 ""
#endif
#ifdef DD3D_STEM_TW
#define DD3D_BF_4 " DD3D_STEM_TW=" DD3D_BF_STR(DD3D_STEM_TW)
#else
#define DD3D_BF_4 ""
#endif
#ifdef DD3D_STEM_WAVES
#define DD3D_BF_5 " DD3D_STEM_WAVES=" DD3D_BF_STR(DD3D_STEM_WAVES)
#else
#define DD3D_BF_5 ""
#endif
#ifdef DD3D_STEM_CHAINS
#define DD3D_BF_6 " DD3D_STEM_CHAINS=" DD3D_BF_STR(DD3D_STEM_CHAINS)
#else
#define DD3D_BF_6 ""
#endif
#ifdef DD3D_ROW_STAMP
#define DD3D_BF_7 " DD3D_ROW_STAMP=" DD3D_BF_STR(DD3D_ROW_STAMP)
#else
#define DD3D_BF_7 ""
#endif
#define DD3D_BUILD_FLAGS DD3D_BF_0 DD3D_BF_1 DD3D_BF_2 DD3D_BF_3 DD3D_BF_4 DD3D_BF_5 DD3D_BF_6 DD3D_BF_7
