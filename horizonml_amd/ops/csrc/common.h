// Common device helpers for the horizonml_amd gfx950 kernels.
// CDNA4-only: wave64, MFMA bf16, LDS-staged tiles. No CUDA compat paths.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>

#include "launch.h"  // ConvP, MagicP, task tables, launcher declarations

#define WAVE 64
#define DEV __device__ __forceinline__

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

using bf16 = __bf16;

DEV float b2f(bf16 x) { return (float)x; }
DEV bf16 f2b(float x) { return (bf16)x; }   // clang emits v_cvt (RNE) on gfx950

// 16-byte vector of 8 bf16 for global loads/stores.
union V8 {
  bf16x8 v;
  uint4 u;
  bf16 e[8];
};

DEV int cdiv(int a, int b) { return (a + b - 1) / b; }

// Block-wide f32 reduction helper over one wave via xor shuffles (wave64).
DEV float wave_reduce_sum(float x) {
  for (int off = 32; off > 0; off >>= 1)
    x += __shfl_xor(x, off, 64);
  return x;
}

// Device side of MagicP (launch.h): q = (umulhi(n, m) + n) >> s.
DEV unsigned fdiv(unsigned n, const MagicP& mg, int i) {
  return mg.d[i] == 1 ? n : (__umulhi(n, mg.m[i]) + n) >> mg.s[i];
}

DEV unsigned fmod(unsigned n, unsigned q, const MagicP& mg, int i) {
  return n - q * mg.d[i];
}

// ---------------------------------- row-major LDS tile, transposed read --
// A K-step tile of (32 reduction rows × TN output columns) staged as it lies
// in memory; the MFMA fragment (8 consecutive reduction rows of one column
// per lane) is fetched with ds_read_b64_tr_b16.  Used by dgrad's KRSC B
// operand, wgrad and the wide classifier head.
//
// Image: row pitch TN*2 bytes, the row's 32-byte chunks (16 columns) XORed
// with a function of the row.  One transposed read serves, per 32-lane
// half, two 4-row blocks 8 rows apart in the same 16 columns (groups g and
// g+1: rows 8g+q and 8g+8+q).  A pitch that is a multiple of 32 B leaves
// rows r and r+8 on the same banks, and a 16-B-odd pitch (the +8 pad of the
// row-major image) always overlaps two of the eight rows, so the rows are
// separated by the swizzle instead: with 128-B rows (TN=64) the row parity
// picks the half of the 256-B bank row and bits {1,3} of the row pick the
// chunk; with 256-B rows (TN=128) bits {0,1,3} do.  The eight rows of a
// half then cover all 64 banks once: conflict-free by the bank rule.  The
// swizzle moves whole 32-byte chunks, so the 16-byte staging stores and
// the 8-byte-aligned transposed reads both stay inside one chunk, and the
// second read of a fragment (rows +4) is the first one's address + 4 rows.
// The wgrad operand tiles ([32 m][k3], [32 m][ko]) use the same image.
template <int TN>
DEV int lds_tr_off(int k, int n) {
  const int f = TN == 64 ? (((k >> 1) & 1) | (((k >> 3) & 1) << 1))
                         : ((k & 3) | (((k >> 3) & 1) << 2));
  return k * TN + ((((n >> 4) ^ f)) << 4) + (n & 15);
}

typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// ds_read_b64_tr_b16.  Needs EXEC all ones: call it from block-uniform
// control flow only, with every lane's address inside the image.
DEV bf16x4 lds_read_tr16(const bf16* sp) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4*)sp);
}
