// gost28147_kernels.hip — batched GOST 28147-89 (include/lcb_gost28147_gpu.h)
// for gfx950: ECB encrypt / decrypt and the MAC (imitovstavka).
//
// The round function (gost28147.h:222-242) is four byte-indexed table
// lookups, so this kernel is table-lookup-bound where every other kernel of
// the project is add/rotate-bound, and the LDS layout decides its speed.
//
// Table.  The reference's four 256 x u32 tables (gost28147.h:494-507) carry 8
// significant bits each, so they pack into ONE 256-word table
//   P[i] = rotl32(t0[i] | t1[i] << 8 | t2[i] << 16 | t3[i] << 24, 11)
// (built on the host), and byte k of the round output is selected from P[x_k]
// with the byte masks rotated by 11 (three v_bitop3_b32).  In LDS the table is
// kept as 32 lane-private copies, word address idx * 32 + (lane & 31):
// ds_read_b32 banks are (addr / 4) % 32 and conflicts are counted per 32-lane
// half, so every lane stays on its own bank whatever the data — no bank
// conflict by construction.  32 KiB per workgroup, 5 workgroups per CU.
//
// ECB (gost28147.h:336-481).  Blocks are independent, so the unit of work is a
// block PAIR (16 bytes), one lane each: a dense 16-B aligned batch moves
// dwordx4 per lane, fully coalesced, and the two independent Feistel chains
// of a lane hide each other's LDS latency.  Fixed layouts divide once per
// wave; ragged layouts search a device-built exclusive prefix of pairs per
// buffer.  Buffers at any byte alignment: aligned dword slots with
// v_alignbyte funnel shifts, byte stores only at a lane's two edge dwords.
// Nothing is read beyond the dword holding a buffer's last processed byte,
// nothing outside a buffer's whole blocks is written.
//
// Encrypt and decrypt differ only in the key order, which the host expands
// into 32 round keys (wave-uniform, SGPRs); LE and BE differ only in the
// load/store byte order (the key swap of gost28147_init_be happens on the
// host).  So there is one ECB kernel and one MAC kernel.
//
// MAC (gost28147.h:244-253, 288-333).  One sequential chain per buffer: one
// lane per buffer, 16 rounds per block, the same LDS table.  A long buffer
// cannot be segmented — each block's input is the previous block's output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gost28147_internal.hpp"

namespace lcbgost {

template <class T>
__device__ __forceinline__ T* gptr(T* p) {
    return (T*)(__attribute__((address_space(1))) T*)p;
}

constexpr uint32_t kCopies = 32;               // lane-private table copies
constexpr uint32_t kTableWords = 256 * kCopies;

// (a & m) | (b & ~m) as ONE v_bitop3_b32 (truth table 0xca with the
// sources weighted 0xf0, 0xcc, 0xaa).  Written in C++ operators the
// compiler re-associates the three selects of a round and the xor into 6
// VALU instructions instead of 4.
__device__ __forceinline__ uint32_t bfi(uint32_t m, uint32_t a, uint32_t b) {
    return __builtin_amdgcn_bitop3_b32(m, a, b, 0xca);
}

// Every workgroup builds its 32 copies from the 1 KiB table (L2 hits):
// consecutive threads write consecutive words.
__device__ __forceinline__ void table_fill(uint32_t* T, const uint32_t* table) {
#pragma unroll 4
    for (uint32_t j = 0; j < kTableWords / 256; ++j) {
        const uint32_t w = j * 256u + threadIdx.x;
        T[w] = gptr(table)[w / kCopies];
    }
    __syncthreads();
}

// rotl32(0xff << 8k, 11), k = 0..2: where byte k of the sbox output lands.
constexpr uint32_t kM0 = 0x0007f800u, kM1 = 0x07f80000u, kM2 = 0xf8000007u;

// gost28147_block32 (gost28147.h:222-229); Tl = table + the lane's copy.
__device__ __forceinline__ uint32_t gost_f(const uint32_t* Tl, uint32_t x) {
    const uint32_t r0 = Tl[(x & 255u) * kCopies];
    const uint32_t r1 = Tl[((x >> 8) & 255u) * kCopies];
    const uint32_t r2 = Tl[((x >> 16) & 255u) * kCopies];
    const uint32_t r3 = Tl[(x >> 24) * kCopies];
    return bfi(kM0, r0, bfi(kM1, r1, bfi(kM2, r2, r3)));
}

// The *_be forms (gost28147.h:372-407, 446-481) swap the two words and the
// bytes of each, on load and on store alike.
__device__ __forceinline__ void be_swap(uint32_t& a, uint32_t& b) {
    const uint32_t t = __builtin_bswap32(b);
    b = __builtin_bswap32(a);
    a = t;
}

// Words of the nb (1 or 2) blocks at s, any alignment.  Misaligned: aligned
// dword slots 0..2nb, the last being the dword that holds the final byte.
__device__ __forceinline__ void load_blocks(const uint8_t* s, uint32_t nb, uint32_t w[4]) {
    const uintptr_t as = reinterpret_cast<uintptr_t>(s);
    if (nb == 2 && (as & 15u) == 0) {
        const uint4 v = *reinterpret_cast<const uint4*>(s);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
        return;
    }
    const uint32_t sh = (uint32_t)(as & 3u), nw = 2u * nb;
    const uint32_t* b = reinterpret_cast<const uint32_t*>(s - sh);
    uint32_t slot[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) slot[k] = ((uint32_t)k < nw || ((uint32_t)k == nw && sh)) ? b[k] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) w[k] = sh ? __builtin_amdgcn_alignbyte(slot[k + 1], slot[k], sh) : slot[k];
}

// Store the nb blocks o[] at d, any alignment: whole dwords where all four
// bytes are this lane's, single bytes in its two edge dwords.
__device__ __forceinline__ void store_blocks(uint8_t* d, uint32_t nb, const uint32_t o[4]) {
    const uintptr_t ad = reinterpret_cast<uintptr_t>(d);
    if (nb == 2 && (ad & 15u) == 0) {
        *reinterpret_cast<uint4*>(d) = make_uint4(o[0], o[1], o[2], o[3]);
        return;
    }
    const uint32_t sh = (uint32_t)(ad & 3u), nw = 2u * nb;
    if (sh == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((uint32_t)k < nw) reinterpret_cast<uint32_t*>(d)[k] = o[k];
        return;
    }
    uint8_t* db = d - sh;  // slot k holds output bytes [4k - sh, 4k - sh + 4)
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        if ((uint32_t)k > nw) continue;
        const uint32_t hi = k < 4 ? o[k] : 0u, lo = k > 0 ? o[k - 1] : 0u;
        const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, 4u - sh);
        if (k >= 1 && (uint32_t)k < nw) {
            *reinterpret_cast<uint32_t*>(db + 4 * k) = v;
        } else {
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j)
                if (k == 0 ? j >= sh : j < sh) db[4 * k + j] = (uint8_t)(v >> (8u * j));
        }
    }
}

// ------------------------------------------------- table upload
// One lane copies the by-value table with compile-time indices (a dynamic
// index into a kernel argument would go through scratch).
__global__ __launch_bounds__(64) void gost28147_table_kernel(GostTable t, uint32_t* out) {
    if (threadIdx.x != 0) return;
    uint4* o = reinterpret_cast<uint4*>(gptr(out));
#pragma unroll
    for (int k = 0; k < 64; ++k) o[k] = make_uint4(t.w[4 * k], t.w[4 * k + 1], t.w[4 * k + 2], t.w[4 * k + 3]);
}

// ------------------------------------------------- ragged: pair prefix
// pair_start[i] = sum_{k<i} pairs(len_k), pair_start[count] = total.  Three
// passes of 1024 buffers per workgroup (4 per thread).
constexpr int kScanPer = 1024;

__device__ __forceinline__ uint64_t wg_inclusive_scan(uint64_t v, uint64_t* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 256; d <<= 1) {
        const uint64_t add = threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
        __syncthreads();
        v += add;
        sh[threadIdx.x] = v;
        __syncthreads();
    }
    return v;
}

__global__ __launch_bounds__(256) void gost28147_scan_reduce(const uint32_t* lengths, uint64_t count,
                                                             uint64_t* parts) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanPer + threadIdx.x * 4u;
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (base + k < count) s += gost_pairs_of(gptr(lengths)[base + k]);
    const uint64_t inc = wg_inclusive_scan(s, sh);
    if (threadIdx.x == 255) gptr(parts)[blockIdx.x] = inc;
}

__global__ __launch_bounds__(256) void gost28147_scan_parts(uint64_t* parts, uint64_t nparts) {
    __shared__ uint64_t sh[256];
    uint64_t carry = 0;
    for (uint64_t b = 0; b < nparts; b += 256) {
        const uint64_t i = b + threadIdx.x;
        const uint64_t v = i < nparts ? gptr(parts)[i] : 0u;
        const uint64_t inc = wg_inclusive_scan(v, sh);
        if (i < nparts) gptr(parts)[i] = carry + inc - v;
        carry += sh[255];
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void gost28147_scan_final(const uint32_t* lengths, uint64_t count,
                                                            const uint64_t* parts, uint64_t* pair_start) {
    __shared__ uint64_t sh[256];
    const uint64_t base = (uint64_t)blockIdx.x * kScanPer + threadIdx.x * 4u;
    uint64_t b[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[k] = base + k < count ? gost_pairs_of(gptr(lengths)[base + k]) : 0u;
        s += b[k];
    }
    const uint64_t inc = wg_inclusive_scan(s, sh);
    uint64_t run = gptr(parts)[blockIdx.x] + inc - s;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (base + k < count) gptr(pair_start)[base + k] = run;
        run += b[k];
        if (base + k + 1 == count) gptr(pair_start)[count] = run;
    }
}

// Largest i with ps[i] <= g0 for a wave-uniform g0 < ps[count] (a buffer
// without a whole block shares its start with the next one and is skipped):
// 64-ary, one vector load of 64 evenly spaced entries per step.
__device__ __forceinline__ uint64_t wave_search(const uint64_t* ps, uint64_t count, uint64_t g0, uint32_t lane) {
    uint64_t lo = 0, hi = count;
    while (hi - lo > 1) {
        const uint64_t step = (hi - lo + 63) >> 6;
        const uint64_t idx = lo + (uint64_t)lane * step;
        const bool le = idx < hi && ps[idx] <= g0;  // a prefix of the lanes: ps is sorted
        const uint32_t k = (uint32_t)__popcll(__ballot(le)) - 1u;  // lane 0 always qualifies
        lo += (uint64_t)k * step;
        const uint64_t nh = lo + step;
        hi = nh < hi ? nh : hi;
    }
    return lo;
}

// Per lane: the buffer holding pair g >= ps[lo]; gallop forward from the
// tile's first buffer, then bisect.
__device__ __forceinline__ uint64_t lane_search(const uint64_t* ps, uint64_t count, uint64_t lo, uint64_t g) {
    uint64_t hi = count;
    for (uint64_t s = 1;; s <<= 1) {
        const uint64_t c = lo + s;
        if (c >= count) break;
        if (ps[c] > g) {
            hi = c;
            break;
        }
        lo = c;
    }
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ps[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// ------------------------------------------------- ECB kernel
__global__ __launch_bounds__(256) void gost28147_ecb_kernel(GostArgs a) {
    __shared__ uint32_t T[kTableWords];
    constexpr uint64_t kTile = 64;  // pairs per wave step = 1 KiB
    uint64_t total = a.total_pairs;
    if (a.lengths) {
        const uint64_t tv = gptr(a.pair_start)[a.count];
        total = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(tv >> 32)) << 32) |
                (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)tv);
    }
    if ((uint64_t)blockIdx.x * (blockDim.x >> 6) * kTile >= total) return;  // whole workgroup idle
    table_fill(T, a.table);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t* Tl = T + (lane & (kCopies - 1u));
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) +
                           (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    const uint64_t ppb = a.ppb;
    const uint64_t gstep = nwaves * kTile;
    uint64_t buf0 = 0, jp0 = 0, sdiv = 0, smod = 0;
    if (!a.lengths) {
        if (total <= 0xffffffffull && gstep <= 0xffffffffull) {  // wave-uniform 32-bit divisions
            buf0 = (uint32_t)(wave0 * kTile) / (uint32_t)ppb;
            sdiv = (uint32_t)gstep / (uint32_t)ppb;
        } else {
            buf0 = (wave0 * kTile) / ppb;
            sdiv = gstep / ppb;
        }
        jp0 = wave0 * kTile - buf0 * ppb;
        smod = gstep - sdiv * ppb;
    }
    for (uint64_t t = wave0; t * kTile < total; t += nwaves) {
        const uint64_t g0 = t * kTile;
        uint64_t g = g0 + lane, buf, jp;
        const bool live = g < total;
        if (!live) g = total - 1;
        if (a.lengths) {
            const uint64_t first = wave_search(gptr(a.pair_start), a.count, g0, lane);
            buf = lane_search(gptr(a.pair_start), a.count, first, g);
            jp = g - gptr(a.pair_start)[buf];
        } else if (ppb >= kTile) {
            jp = jp0 + lane;
            buf = buf0;
            if (jp >= ppb) {
                jp -= ppb;
                ++buf;
            }
            if (buf >= a.count) buf = a.count - 1;
        } else {
            const uint32_t r = (uint32_t)jp0 + lane;
            const uint32_t k = r / (uint32_t)ppb;
            buf = buf0 + k;
            jp = r - k * (uint32_t)ppb;
            if (buf >= a.count) buf = a.count - 1;
        }
        const uint64_t off = a.offsets ? gptr(a.offsets)[buf] : buf * a.stride;
        const uint64_t nblk = (a.lengths ? gptr(a.lengths)[buf] : a.fixed_len) >> 3;
        const uint64_t b0 = 2u * jp;
        const uint32_t nb = (live && nblk > b0) ? (nblk - b0 < 2u ? 1u : 2u) : 0u;
        if (nb) {
            uint32_t w[4];
            load_blocks(gptr(a.src) + off + 8u * b0, nb, w);
            if (!a.copy_only) {
                if (a.be) {
                    be_swap(w[0], w[1]);
                    be_swap(w[2], w[3]);
                }
                uint32_t n1 = w[0], n2 = w[1], m1 = w[2], m2 = w[3];  // two independent chains
#pragma unroll
                for (int r = 0; r < 32; r += 2) {  // gost28147.h:198-217
                    n2 ^= gost_f(Tl, n1 + a.ks[r]);
                    m2 ^= gost_f(Tl, m1 + a.ks[r]);
                    n1 ^= gost_f(Tl, n2 + a.ks[r + 1]);
                    m1 ^= gost_f(Tl, m2 + a.ks[r + 1]);
                }
                w[0] = n2; w[1] = n1; w[2] = m2; w[3] = m1;  // gost28147.h:266-268
                if (a.be) {
                    be_swap(w[0], w[1]);
                    be_swap(w[2], w[3]);
                }
            }
            store_blocks(gptr(a.dst) + off + 8u * b0, nb, w);
        }
        if (!a.lengths) {
            buf0 += sdiv;
            jp0 += smod;
            if (jp0 >= ppb) {
                jp0 -= ppb;
                ++buf0;
            }
        }
    }
}

// ------------------------------------------------- MAC kernel
__device__ __forceinline__ void mac_block(const GostArgs& a, const uint32_t* Tl, uint32_t& m0, uint32_t& m1,
                                          uint32_t w0, uint32_t w1) {
    if (a.be) be_swap(w0, w1);
    m0 ^= w0;
    m1 ^= w1;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {  // gost28147.h:244-253
        m1 ^= gost_f(Tl, m0 + a.ks[r]);
        m0 ^= gost_f(Tl, m1 + a.ks[r + 1]);
    }
}

__global__ __launch_bounds__(256) void gost28147_mac_kernel(GostArgs a) {
    __shared__ uint32_t T[kTableWords];
    table_fill(T, a.table);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t* Tl = T + (lane & (kCopies - 1u));
    const uint64_t wave0 = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nwaves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t t = wave0; t * 64u < a.count; t += nwaves) {
        const uint64_t i = t * 64u + lane;
        if (i >= a.count) continue;
        const uint64_t off = a.offsets ? gptr(a.offsets)[i] : i * a.stride;
        const uint32_t nblk = (a.lengths ? gptr(a.lengths)[i] : a.fixed_len) >> 3;
        const uint8_t* s = gptr(a.src) + off;
        uint32_t m0 = 0, m1 = 0;
        for (uint32_t j = 0; j < nblk; j += 2) {
            const uint32_t nb = nblk - j < 2u ? 1u : 2u;
            uint32_t w[4];
            load_blocks(s + 8ull * j, nb, w);
            mac_block(a, Tl, m0, m1, w[0], w[1]);
            if (nb == 2) mac_block(a, Tl, m0, m1, w[2], w[3]);
        }
        if (a.be) {  // gost28147_final_be (gost28147.h:555-556)
            m0 = __builtin_bswap32(m0);
            m1 = __builtin_bswap32(m1);
        }
        uint8_t* o = gptr(a.dst) + i * a.mac_size;
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b)
            if (b < a.mac_size) o[b] = (uint8_t)((b < 4 ? m0 : m1) >> (8u * (b & 3u)));
    }
}

// ------------------------------------------------- launchers
static uint32_t cu_count() {
    static int cache[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cache[dev] <= 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 256;
        cache[dev] = cus;
    }
    return (uint32_t)cache[dev];
}

// 32 KiB of LDS per workgroup: 5 workgroups are resident per CU.
constexpr uint64_t kWgPerCu = 5;

void launch_gost_table(const GostTable& t, uint32_t* dtable, hipStream_t s) {
    hipLaunchKernelGGL(gost28147_table_kernel, dim3(1), dim3(64), 0, s, t, dtable);
}

void launch_gost_ecb(const GostArgs& a, uint64_t nparts, uint64_t* parts, uint64_t* pair_start, hipStream_t s) {
    GostArgs k = a;
    const uint64_t resident = (uint64_t)cu_count() * kWgPerCu;
    uint64_t grid;
    if (a.lengths) {
        const unsigned nb = (unsigned)((a.count + kScanPer - 1) / kScanPer);
        hipLaunchKernelGGL(gost28147_scan_reduce, dim3(nb), dim3(256), 0, s, a.lengths, a.count, parts);
        hipLaunchKernelGGL(gost28147_scan_parts, dim3(1), dim3(256), 0, s, parts, nparts);
        hipLaunchKernelGGL(gost28147_scan_final, dim3(nb), dim3(256), 0, s, a.lengths, a.count,
                           (const uint64_t*)parts, pair_start);
        k.pair_start = pair_start;
        // The total is known on the device only: workgroups past it leave
        // before they build their table.
        grid = 2 * resident;
    } else {
        // A wave amortises its workgroup's table build over ~8 tiles of
        // 1 KiB; small batches spread over the CUs first.
        const uint64_t tiles = (a.total_pairs + 63) / 64, wgs = (tiles + 3) / 4;
        grid = std::max<uint64_t>((wgs + 7) / 8, std::min<uint64_t>(wgs, resident));
        grid = std::min<uint64_t>(grid, 4 * resident);
    }
    hipLaunchKernelGGL(gost28147_ecb_kernel, dim3((unsigned)std::max<uint64_t>(grid, 1)), dim3(256), 0, s, k);
}

void launch_gost_mac(const GostArgs& a, hipStream_t s) {
    const uint64_t wgs = (a.count + 255) / 256;
    const uint64_t grid = std::min<uint64_t>(wgs, 4ull * cu_count() * kWgPerCu);
    hipLaunchKernelGGL(gost28147_mac_kernel, dim3((unsigned)std::max<uint64_t>(grid, 1)), dim3(256), 0, s, a);
}

}  // namespace lcbgost
