// Shared device helpers of the kernels that stage 32-frame rows through LDS-DMA rings and write with buffer stores
// (gemm_conv.hip, gemm_x3.hip, pw_bwd.hip, convt_bwd.hip, gru.hip).
#pragma once
#include "common.hpp"

namespace {

// destination operand of __builtin_amdgcn_global_load_lds
typedef __attribute__((address_space(3))) void* lds_ptr_t;

// s_waitcnt vmcnt(n) for a run-time n in 0 .. MAXN (the instruction takes an immediate, so this is a jump table; a ring
// picks the MAXN that covers its counts: 31 or 60), vmcnt(0) beyond.  Not the rounding wait_vmcnt of gemm_common.hpp.
#define VMCNT_0_31_(W_)                                                                                                \
    W_(0) W_(1) W_(2) W_(3) W_(4) W_(5) W_(6) W_(7) W_(8) W_(9) W_(10) W_(11) W_(12) W_(13) W_(14) W_(15)             \
    W_(16) W_(17) W_(18) W_(19) W_(20) W_(21) W_(22) W_(23) W_(24) W_(25) W_(26) W_(27) W_(28) W_(29) W_(30) W_(31)
#define VMCNT_32_60_(W_)                                                                                               \
    W_(32) W_(33) W_(34) W_(35) W_(36) W_(37) W_(38) W_(39) W_(40) W_(41) W_(42) W_(43) W_(44) W_(45) W_(46) W_(47)   \
    W_(48) W_(49) W_(50) W_(51) W_(52) W_(53) W_(54) W_(55) W_(56) W_(57) W_(58) W_(59) W_(60)
#define VMCNT_CASE_(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
template <int MAXN>
__device__ __forceinline__ void wait_vmcnt_exact(int n) {
    static_assert(MAXN == 31 || MAXN == 60, "ranges with a case list");
    if constexpr (MAXN == 31) {
        switch (n) {
            VMCNT_0_31_(VMCNT_CASE_)
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
    } else {
        switch (n) {
            VMCNT_0_31_(VMCNT_CASE_) VMCNT_32_60_(VMCNT_CASE_)
            default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
        }
    }
}
#undef VMCNT_CASE_
#undef VMCNT_32_60_
#undef VMCNT_0_31_

// swizzled float offset of 16-byte piece `pc` (0..7) of row `r` inside a slot of 32-frame rows: the DMA source address
// carries the same XOR, so a column of pieces spreads over all banks
__device__ __forceinline__ int swz_off(int r, int pc) { return r * 32 + 4 * (pc ^ ((r >> 1) & 7)); }

// Global rows as buffer resource (SGPR descriptor of a uniform base) + uniform SGPR row offset + one per-lane VGPR
// offset: 64-bit per-row addresses for 16 rows x 3 tensors would not fit the register budget next to the W^T fragments,
// and -- unlike hand-written asm loads -- the compiler tracks these, so a value is never copied or spilled before it has
// arrived (an earlier inline-asm version produced a wrong 32x32 tile about once in a hundred launches under register
// pressure).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* base) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0x7fffffff, 0x00020000);
}

// a wave-uniform value the compiler cannot prove uniform
__device__ __forceinline__ int wave_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// a wave-uniform pointer, as two readfirstlane'd halves: a descriptor built from it stays in SGPRs (no waterfall loop
// around the buffer operations that use it)
template <typename T>
__device__ __forceinline__ T* wave_uniform_ptr(T* p) {
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return (T*)(((unsigned long long)hi << 32) | lo);
}

// 4 / 8 / 16-byte row pieces (float, f32x2, f32x4) through a buffer resource: per-lane byte offset + uniform byte offset.
// Keep soff = 0 for the 16-byte stores unless two wait states separate the store from the next write to its data registers.
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void buffer_store_row(__amdgpu_buffer_rsrc_t r, int voff, int soff, float v) {
    __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buffer_store_row(__amdgpu_buffer_rsrc_t r, int voff, int soff, f32x2 v) {
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, 0);
}
__device__ __forceinline__ void buffer_store_row(__amdgpu_buffer_rsrc_t r, int voff, int soff, f32x4 v) {
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, soff, 0);
}
// Keeps a scalar fp32 result scalar: plain -O3 packs adjacent scalar adds into v_pk_add_f32, and beside MFMAs a packed f32
// operation costs more than the two scalar ones it replaces (same result bits either way).  No instruction is emitted, and the
// arithmetic itself stays visible to the compiler, which places the wait states an MFMA result needs before a vector
// instruction may read it -- an add written in inline assembly does not get them.
__device__ __forceinline__ float keep_scalar(float x) {
    asm("" : "+v"(x));
    return x;
}

}  // namespace
