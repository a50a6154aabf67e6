// hb_regs.hip.h - register-block helpers shared by the device code: one quad (4 lanes) holds one 64-byte
// HyperLogLog<64> counter, lane q the registers [16q, 16q+16) as a uint4; byte-wise max = HyperLogLog::merge
// (crates/core/src/hyperloglog.rs:4531-4535) on even/odd bytes with v_pk_max_u16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hbk {

// ---- quad helpers ---------------------------------------------------------------------
template <int J>
__device__ __forceinline__ uint32_t quad_bcast(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, J * 0x55, 0xF, 0xF, true);
}
template <int CTRL>
__device__ __forceinline__ uint32_t quad_perm(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xF, 0xF, true);
}
// bit g of the result = any lane of quad g voted (ballot folded 4:1); scalar ALU work
__device__ __forceinline__ uint32_t pack16(uint64_t b)
{
    b |= b >> 1;
    b |= b >> 2;
    b &= 0x1111111111111111ull;
    b = (b | (b >> 3)) & 0x0303030303030303ull;
    b = (b | (b >> 6)) & 0x000F000F000F000Full;
    b = (b | (b >> 12)) & 0x000000FF000000FFull;
    b = (b | (b >> 24)) & 0xFFFFull;
    return (uint32_t)b;
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pkmax(uint32_t a, uint32_t b)
{
    us2 x = __builtin_bit_cast(us2, a), y = __builtin_bit_cast(us2, b);
    us2 z = __builtin_elementwise_max(x, y);
    return __builtin_bit_cast(uint32_t, z);
}

// 16 registers of one lane kept as even/odd bytes so that one merge is 1 AND + 2 v_pk_max_u16 per word: the even bytes
// are compared as clean 16-bit lanes (0x00FF00FF masked); the odd bytes as the HIGH bytes of the unmasked 16-bit lanes -
// a lane's maximum has the larger high byte whatever the low bytes are, so o[] carries garbage in its low bytes until
// acc_value() masks it once.
struct Acc {
    uint32_t e[4], o[4];
};
__device__ __forceinline__ void acc_zero(Acc &a)
{
#pragma unroll
    for (int k = 0; k < 4; k++) a.e[k] = a.o[k] = 0;
}
__device__ __forceinline__ void acc_merge(Acc &a, const uint4 &r)
{
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
        a.e[k] = pkmax(a.e[k], w[k] & 0x00FF00FFu);
        a.o[k] = pkmax(a.o[k], w[k]);
    }
}
__device__ __forceinline__ uint4 acc_value(const Acc &a)
{
    return make_uint4(a.e[0] | (a.o[0] & 0xFF00FF00u), a.e[1] | (a.o[1] & 0xFF00FF00u), a.e[2] | (a.o[2] & 0xFF00FF00u),
                      a.e[3] | (a.o[3] & 0xFF00FF00u));
}
__device__ __forceinline__ bool u4_ne(const uint4 &a, const uint4 &b)
{
    return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) != 0;
}
// a >= b in each of the 16 registers: the byte-wise maximum of the two (even and odd bytes as 16-bit lanes, as in acc_merge) is a
__device__ __forceinline__ bool counter_ge(const uint4 &a, const uint4 &b)
{
    const uint32_t x[4] = {a.x, a.y, a.z, a.w}, y[4] = {b.x, b.y, b.z, b.w};
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t xe = x[k] & 0x00FF00FFu, xo = (x[k] >> 8) & 0x00FF00FFu;
        diff |= (pkmax(xe, y[k] & 0x00FF00FFu) ^ xe) | (pkmax(xo, (y[k] >> 8) & 0x00FF00FFu) ^ xo);
    }
    return diff == 0;
}

// the accumulator >= b in each of the 16 registers, without acc_value(): the even bytes are clean 16-bit lanes; an odd byte is the high
// byte of its lane of o[], which is >= the lane of b with the low byte cleared exactly when its high byte is >= b's
__device__ __forceinline__ bool acc_ge(const Acc &a, const uint4 &b)
{
    const uint32_t y[4] = {b.x, b.y, b.z, b.w};
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) diff |= (pkmax(a.e[k], y[k] & 0x00FF00FFu) ^ a.e[k]) | (pkmax(a.o[k], y[k] & 0xFF00FF00u) ^ a.o[k]);
    return diff == 0;
}

// the one register HyperLogLog::default(); add_u128(id) sets (hyperloglog.rs:4385-4400 with FastHasher :4311-4313; only the low 64 bits of
// the id are hashed), as index | value << 8 - the entry format of src_jp / self_jp
__device__ __forceinline__ uint16_t initial_register_jp(uint64_t id_low)
{
    const uint64_t hash = id_low * 11400714819323198549ull;
    const uint32_t j = (uint32_t)(hash >> 58);
    const uint64_t w = hash << 6;
    const uint32_t pval = (w == 0 ? 64u : (uint32_t)__clzll((long long)w)) + 1u;
    return (uint16_t)(j | (pval << 8));
}
// lane q's quarter (registers 16 q .. 16 q + 15) of the counter that entry describes
__device__ __forceinline__ uint4 counter_quarter_of_jp(uint32_t jp, int q)
{
    const uint32_t j = jp & 63u, pval = jp >> 8;
    uint32_t ww[4] = {0, 0, 0, 0};
    if (pval && (int)(j >> 4) == q) ww[(j & 15u) >> 2] = pval << (8 * (j & 3u));
    return make_uint4(ww[0], ww[1], ww[2], ww[3]);
}

} // namespace hbk
