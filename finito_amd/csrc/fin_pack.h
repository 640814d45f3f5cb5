// fin_pack.h -- ASCII bases -> the 16-byte chunks of a step: the code the ingest kernel (fin_pack.hip) and the fast pre-pass's fused ingest
// (fin_prepass.hip) share, so that both write the same bits.
// A chunk = 32 bases of one strand as {u64 2-bit codes (A0 C1 G2 T3, base j at bits 2j), u32 validity bits, u32 0}.  Case-insensitive; any other
// byte is an invalid base, whose code is 0.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace fin_pack {
// 0x80 in every byte of v that is zero (exact: no borrow crosses a byte)
__device__ __forceinline__ uint32_t zero_bytes(uint32_t v) { return ~(((v & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | v) & 0x80808080u; }

// four ASCII bases (byte j = position j) -> 8 code bits (2 per base) and 4 validity bits
__device__ __forceinline__ void pack4(uint32_t w, bool comp, uint32_t& codes, uint32_t& valid) {
    const uint32_t x = w & 0xDFDFDFDFu;                                   // upper case
    const uint32_t r = (x >> 1) & 0x03030303u;                            // A 0, C 1, T 2, G 3
    // the one letter a byte with these two bits can be: 'A' + {0, 2, 0x13, 6}[r], byte-wise (0/1 bytes times small constants: no carry)
    const uint32_t b0 = r & 0x01010101u, b1 = (r >> 1) & 0x01010101u;
    const uint32_t expect = 0x41414141u + (b0 << 1) + b1 * 0x13u - (b0 & b1) * 0x0Fu;
    const uint32_t ok = zero_bytes(x ^ expect) >> 7;                      // 1 in every byte that is a base
    uint32_t y = r ^ b1;                                                  // A 0, C 1, G 2, T 3
    if (comp) y ^= 0x03030303u;
    y &= ok * 3u;                                                         // an invalid base has code 0
    codes = (y * 0x01041040u) >> 24;                                      // byte j's two bits -> bits 2j
    valid = ((ok * 0x01020408u) >> 24) & 0xFu;                            // byte j's flag -> bit j
}

// chunk ci of strand s (false: forward, true: reverse complement) of the read of `len` bases at `read` (ci < ceil(len / 32)).  Reads a 32-byte
// window that may overhang the read by up to 31 bytes at either end: the bases buffer has guard bytes around it.
__device__ __forceinline__ void make_chunk(const uint8_t* read, uint32_t len, uint32_t ci, bool s, uint64_t& codes, uint32_t& valid) {
    const uint32_t p0 = ci * 32u;                       // first position of the chunk in strand coordinates
    const uint32_t cnt = len - p0 < 32u ? len - p0 : 32u;
    // forward: bytes p0 ..; reverse: window [len-p0-32, len-p0) read backwards
    const uint8_t* src = s ? read + len - p0 - 32 : read + p0;
    uint4 va, vb;
    __builtin_memcpy(&va, src, 16); __builtin_memcpy(&vb, src + 16, 16);
    const uint32_t wds[8] = {va.x, va.y, va.z, va.w, vb.x, vb.y, vb.z, vb.w};
    codes = 0; valid = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) {
        // strand positions 4q..4q+3: forward = dword q; reverse = dword 7-q with its bytes reversed, complemented
        const uint32_t wd = s ? __builtin_bswap32(wds[7 - q]) : wds[q];
        uint32_t c8, v4;
        pack4(wd, s, c8, v4);
        codes |= (uint64_t)c8 << (8 * q);
        valid |= v4 << (4 * q);
    }
    const uint32_t keep = cnt >= 32u ? 0xFFFFFFFFu : ((1u << cnt) - 1u);
    valid &= keep;
    // codes of invalid positions are 0: spread the 32 validity bits to 2 bits each
    uint64_t m = valid;
    m = (m | (m << 16)) & 0x0000FFFF0000FFFFull; m = (m | (m << 8)) & 0x00FF00FF00FF00FFull;
    m = (m | (m << 4)) & 0x0F0F0F0F0F0F0F0Full; m = (m | (m << 2)) & 0x3333333333333333ull;
    m = (m | (m << 1)) & 0x5555555555555555ull;
    codes &= m | (m << 1);
}

// the reverse complement of 32 bases (2-bit codes, the first base in the low bits)
__device__ __forceinline__ uint64_t revcomp32(uint64_t x) {
    uint64_t r = __brevll(x);
    r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
    return ~r;
}
}  // namespace fin_pack
