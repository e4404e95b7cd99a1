// Shared device-side idioms of the kernels: the int8 MFMA register types, LDS-DMA issue, the wave-uniform LDS base, the cursor of the constexpr LDS plans, the XCD-aware work order and bf16 bit conversions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vc {

// Operand and accumulator registers of v_mfma_i32_32x32x32_i8: lane 32 h + c holds 16 operand bytes [32 kk + 16 h, +16) of
// row c at k-step kk, and accumulator element 4 q + i is row 8 q + 4 h + i against column c.
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// LDS-DMA (global_load_lds): each lane copies 16 (or 4) bytes from its own global address to LDS at the wave-uniform
// byte address `lds_dst` + lane * 16 (or 4).  M0 holds the LDS destination; the compiler reserves it and does not
// preserve it around an asm statement, so each statement saves M0, sets it, issues the load and restores M0 itself.
// The copies are invisible to hipcc's s_waitcnt bookkeeping: the caller waits for them with its own vmcnt count, then
// a barrier, before any LDS read of the data.  `lds_dst` must be an SGPR value (see lds_addr).

// Per-lane 64-bit source address.
__device__ __forceinline__ void lds_dma16(const void* vaddr, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(vaddr), "s"(lds_dst)
      : "memory");
}

// Wave-uniform base in an SGPR pair + per-lane 32-bit byte offset: one VGPR per lane instead of a 64-bit address.
__device__ __forceinline__ void lds_dma16(const void* sbase, uint32_t voffset, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %3\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dwordx4 %1, %2\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voffset), "s"(sbase), "s"(lds_dst)
      : "memory");
}

// 4 bytes per lane (inactive lanes copy nothing).
__device__ __forceinline__ void lds_dma4(const void* vaddr, uint32_t lds_dst) {
  uint32_t keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\t"
      "s_mov_b32 m0, %2\n\t"
      "s_nop 0\n\t"
      "global_load_lds_dword %1, off\n\t"
      "s_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(vaddr), "s"(lds_dst)
      : "memory");
}

// LDS byte address of a __shared__ object.
__device__ __forceinline__ uint32_t lds_offset(const void* p) {
  return (uint32_t)(size_t)(__attribute__((address_space(3))) const void*)p;
}

// The same, made provably wave-uniform so that it can feed an "s" operand.
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)__builtin_amdgcn_readfirstlane((int)lds_offset(p));
}

// For a kernel's constexpr LDS plan (one function that kernel and host both evaluate): hands out consecutive regions,
// each at its alignment; offsets are in bytes from the start of LDS and `at` ends as the size.
struct LdsCursor {
  uint32_t at;
  __host__ __device__ constexpr uint32_t take(uint32_t bytes, uint32_t align = 4) {
    at = (at + align - 1) / align * align;
    const uint32_t off = at;
    at += bytes;
    return off;
  }
};

// XCD-aware work order: the 8 XCDs take workgroups round-robin (blocks b and b + 8 share an L2, b and b + 1 never do), so
// launch slot `slot` of `n_tiles` gets the tile that gives each XCD a contiguous run of tiles: what an XCD works on at one
// time is then neighbouring tiles, whose common operand (the staged GEMMs' x rows, the attention units' K / V) is in its L2.
// A bijection of [0, n_tiles) for every n_tiles; placement is not a contract, so this may change speed only.
__device__ __forceinline__ int xcd_tile(int slot, int n_tiles) {
  const int xcd = slot & 7, idx = slot >> 3;
  const int q = n_tiles >> 3, r = n_tiles & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }

// Round to nearest even; NaN stays NaN (quiet bit set, so the truncated mantissa cannot become zero).
__device__ __forceinline__ uint16_t f32_to_bf16(float v) {
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

}  // namespace vc
