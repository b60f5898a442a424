// BGZF members inflated on the device (HULK_INGEST_DEVICE_INFLATE, hulk_bgzf_inflate).
//
// A bgzip'd file is a chain of independent gzip members of at most 64 KiB of text whose headers carry their compressed size
// (hulk_bgzf.h, bgzf::member_size): the host frames a batch of members from the compressed bytes alone, the device inflates
// every member into its own slice of the batch's text and checks it, and the host reads one status record per member.
//
// k_bgzf_inflate: one wave64 workgroup per member.  All 64 lanes walk the DEFLATE stream together and identically — same bit
// buffer, same table lookups (broadcast reads of LDS) — so the decode's control flow is uniform without any exchange; the lanes
// part ways only to write: a literal by lane 0, a match's bytes by all lanes at once (byte j of a match with distance d < its
// length is read from j mod d behind its start: every read lies in front of the match).  The text of the member is built in
// a 64 KiB window in LDS, its CRC-32 taken by the lanes over 64 slices (combined with GF(2) powers of x, zlib's
// crc32_combine), then written to HBM coalesced.  The compressed bytes are read as 256-byte rows of dwords held one per lane
// and broadcast with a shuffle.  Decode tables: a 10 / 8 / 7-bit primary lookup for literal-length / distance / code-length
// codes, longer codes by the canonical walk (counts and symbols sorted by length); code-length histograms and ranks by ballots.
//
// Safety: every read of the compressed batch is of a dword inside the buffer (in_bytes rounded up), every write of text is
// inside [out_off, out_off + isize) of a member whose slice the kernel first checks against out_cap; every loop is bounded by
// the text produced (<= ISIZE) or by the bits consumed (checked against the member's payload end).  A malformed member ends
// in a status code.  Strictness is that of the host decoder (fast_inflate.h): over-subscribed and incomplete codes are refused
// (a lone 1-bit code and an empty distance code excepted), as are symbols 286/287 and distances 30/31.
#include <errno.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/hulk_hip.h"
#include "hulk_bgzf.h"

namespace hulk {
namespace bgzf {

const char *status_text(uint32_t st) {
    static const char *const T[ST_COUNT] = {
        "ok", "invalid block type", "invalid or over-subscribed Huffman code", "invalid literal/length or distance symbol",
        "distance before the start of the member", "output longer than ISIZE", "output shorter than ISIZE", "payload exhausted",
        "deflate end not at the payload end", "CRC-32 mismatch", "stored block length check failed", "member outside the batch"};
    return st < ST_COUNT ? T[st] : "unknown status";
}

namespace {

constexpr int LB = 10, DB = 8, CB = 7;          // primary lookup bits: literal/length, distance, code-length codes
constexpr uint32_t POLY = 0xedb88320u;          // CRC-32, reflected
constexpr uint16_t LONG = 0x8000;               // lookup entry: the code is longer than the primary bits

__constant__ uint16_t c_lbase[29] = {3,4,5,6,7,8,9,10,11,13,15,17,19,23,27,31,35,43,51,59,67,83,99,115,131,163,195,227,258};
__constant__ uint8_t c_lext[29] = {0,0,0,0,0,0,0,0,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,4,5,5,5,5,0};
__constant__ uint16_t c_dbase[30] = {1,2,3,4,5,7,9,13,17,25,33,49,65,97,129,193,257,385,513,769,1025,1537,2049,3073,4097,6145,8193,12289,16385,24577};
__constant__ uint8_t c_dext[30] = {0,0,0,0,1,1,2,2,3,3,4,4,5,5,6,6,7,7,8,8,9,9,10,10,11,11,12,12,13,13};
__constant__ uint8_t c_order[19] = {16,17,18,0,8,7,9,6,10,5,11,4,12,3,13,2,14,1,15};

// x^(2^k) mod P, k = 0..31 (zlib's x2n_table: x^1, then each the square of the one before)
__constant__ uint32_t c_x2n[32] = {
    0x40000000,0x20000000,0x08000000,0x00800000,0x00008000,0xedb88320,0xb1e6b092,0xa06a2517,0xed627dae,0x88d14467,0xd7bbfe6a,
    0xec447f11,0x8e7ea170,0x6427800e,0x4d47bae0,0x09fe548f,0x83852d0f,0x30362f1a,0x7b5a9cc3,0x31fec169,0x9fec022a,0x6c8dedc4,
    0x15d6874d,0x5fde7a4e,0xbad90e37,0x2e4e5eef,0x4eaba214,0xa8a472c0,0x429a969e,0x148d302a,0xc40ba6d0,0xc4e22c3c};

struct Lds {
    uint32_t win[(MAX_ISIZE >> 2) + 2];         // the member's text (+ a dword of slack for the unaligned write-out)
    uint32_t crctab[256];
    uint32_t x2n[32];
    uint16_t lut_l[1 << LB], lut_d[1 << DB], lut_c[1 << CB];
    uint16_t cnt_l[16], cnt_d[16], cnt_c[16];
    uint16_t sym_l[288], sym_d[32], sym_c[20];
    uint16_t first[16], offs[16], run[16];      // table build scratch
    uint16_t lbase[29], dbase[30];
    uint8_t lext[29], dext[30], order[19];
    uint8_t lens[288 + 32], clens[20];
};

__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1) ? (b >> 1) ^ POLY : b >> 1;
    }
    return p;
}
// x^(n * 2^k) mod P
__device__ __forceinline__ uint32_t x2nmodp(uint32_t n, unsigned k, const uint32_t *x2n) {
    uint32_t p = 0x80000000u;
    while (n) {
        if (n & 1) p = multmodp(x2n[k & 31], p);
        n >>= 1; k++;
    }
    return p;
}

// the compressed bytes, LSB first: a 64-bit buffer refilled a dword at a time from a row of 64 dwords held one per lane
struct Bits {
    const uint32_t *in32; uint32_t nwords;
    uint64_t bb; int bc; uint32_t nxt, cbase, row; int lane;
    __device__ __forceinline__ void refill() {
        if (bc < 32) {
            if (nxt - cbase >= 64u) { cbase = nxt; const uint32_t i = cbase + (uint32_t)lane; row = i < nwords ? in32[i] : 0u; }
            const uint32_t w = (uint32_t)__shfl((int)row, (int)(nxt - cbase));
            bb |= (uint64_t)w << bc; bc += 32; nxt++;
        }
    }
    __device__ __forceinline__ void seek(uint64_t bit) {
        nxt = (uint32_t)(bit >> 5); cbase = nxt - 64u; bb = 0; bc = 0;
        refill(); drop((int)(bit & 31)); refill();
    }
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)bb & ((1u << n) - 1u); }
    __device__ __forceinline__ void drop(int n) { bb >>= n; bc -= n; }
    __device__ __forceinline__ uint32_t take(int n) { const uint32_t v = peek(n); drop(n); return v; }
    __device__ __forceinline__ uint64_t pos() const { return (uint64_t)nxt * 32u - (uint64_t)bc; }
};

// canonical decode tables for lens[0..n) (what: 0 literal/length, 1 distance, 2 code-length codes); all lanes
__device__ uint32_t build(Lds &S, const uint8_t *lens, int n, int B, int what, uint16_t *lut, uint16_t *cnt, uint16_t *sym, int lane) {
    uint32_t mine = 0;
    for (int c = 0; c < n; c += 64) {
        const int s = c + lane;
        const int l = s < n ? lens[s] : 0;
        for (int L = 1; L <= 15; L++) {
            const uint64_t m = __ballot(l == L);
            if (lane == L) mine += (uint32_t)__popcll(m);
        }
    }
    __syncthreads();
    if (lane < 16) cnt[lane] = (uint16_t)(lane ? mine : 0);
    __syncthreads();
    int left = 1, total = 0, code = 0, off = 0, prev = 0, myfirst = 0, myoff = 0;
    for (int L = 1; L <= 15; L++) {
        const int c = cnt[L];
        left = (left << 1) - c;
        if (left < 0) return ST_BAD_CODE;                           // over-subscribed
        total += c;
        code = (code + prev) << 1;
        if (lane == L) { myfirst = code; myoff = off; }
        off += c; prev = c;
    }
    for (int i = lane; i < (1 << B); i += 64) lut[i] = 0;
    if (total == 0) { __syncthreads(); return what == 1 ? ST_OK : ST_BAD_CODE; }   // (no distance codes: a block of literals)
    if (left > 0 && !(what != 2 && total == 1 && cnt[1] == 1)) return ST_BAD_CODE;  // incomplete (a lone 1-bit code is allowed)
    if (lane < 16) { S.first[lane] = (uint16_t)myfirst; S.offs[lane] = (uint16_t)myoff; S.run[lane] = 0; }
    __syncthreads();
    const uint64_t lt = (1ull << lane) - 1ull;
    for (int c = 0; c < n; c += 64) {
        const int s = c + lane;
        const int l = s < n ? lens[s] : 0;
        int rank = 0; uint32_t add = 0;
        for (int L = 1; L <= 15; L++) {
            const uint64_t m = __ballot(l == L);
            if (l == L) rank = __popcll(m & lt);
            if (lane == L) add = (uint32_t)__popcll(m);
        }
        const int prior = l ? S.run[l] : 0;
        __syncthreads();
        if (lane >= 1 && lane < 16) S.run[lane] = (uint16_t)(S.run[lane] + add);
        if (l) {
            const int k = prior + rank;
            sym[S.offs[l] + k] = (uint16_t)s;
            const uint32_t rev = __brev((uint32_t)(S.first[l] + k)) >> (32 - l);
            if (l <= B) {
                const uint16_t e = (uint16_t)((l << 9) | s);
                for (uint32_t i = rev; i < (1u << B); i += 1u << l) lut[i] = e;
            } else {
                lut[rev & ((1u << B) - 1u)] = LONG;
            }
        }
        __syncthreads();
    }
    return ST_OK;
}

// one symbol; -1 = no such code
__device__ __forceinline__ int decode(Bits &r, const uint16_t *lut, const uint16_t *cnt, const uint16_t *sym, int B) {
    r.refill();                                                      // >= 32 bits: the longest code and its extra bits
    const uint32_t e = lut[r.peek(B)];
    if (!(e & LONG)) {
        const int len = (e >> 9) & 15;
        if (len == 0) return -1;
        r.drop(len);
        return (int)(e & 511);
    }
    int code = 0, first = 0, index = 0;
    for (int L = 1; L <= 15; L++) {
        code |= (int)r.take(1);
        const int count = cnt[L];
        if (code - count < first) return sym[index + (code - first)];
        index += count; first += count; first <<= 1; code <<= 1;
    }
    return -1;
}

__device__ uint32_t inflate_member(Lds &S, const DevMember &M, const uint8_t *in, uint64_t in_bytes, uint32_t *out_pos, int lane) {
    const uint64_t pend = M.in_off + M.in_len, end_bits = pend * 8;
    uint8_t *win = (uint8_t *)S.win;
    Bits r;
    r.in32 = (const uint32_t *)in; r.nwords = (uint32_t)((in_bytes + 3) / 4); r.lane = lane;
    r.seek(M.in_off * 8);
    uint32_t pos = 0;
    bool last = false, fixed = false;
    do {
        if (r.pos() + 3 > end_bits) return ST_EXHAUSTED;
        r.refill();
        last = r.take(1) != 0;
        const uint32_t type = r.take(2);
        if (type == 0) {                                              // stored
            const uint64_t at = (r.pos() + 7) / 8;
            if ((at + 4) * 8 > end_bits) return ST_EXHAUSTED;
            r.seek(at * 8);
            const uint32_t len = r.take(16);
            r.refill();
            const uint32_t nlen = r.take(16);
            if (len != (~nlen & 0xffffu)) return ST_STORED_LEN;
            const uint64_t src = at + 4;
            if (src + len > pend) return ST_EXHAUSTED;
            if (pos + len > M.isize) return ST_TOO_LONG;
            for (uint32_t j = (uint32_t)lane; j < len; j += 64) win[pos + j] = in[src + j];
            pos += len;
            r.seek((src + len) * 8);
            continue;
        }
        if (type == 3) return ST_BLOCK_TYPE;
        uint32_t st;
        if (type == 1) {                                              // fixed codes
            if (!fixed) {
                for (int i = lane; i < 288 + 32; i += 64) S.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5);
                __syncthreads();
                if ((st = build(S, S.lens, 288, LB, 0, S.lut_l, S.cnt_l, S.sym_l, lane)) != ST_OK) return st;
                if ((st = build(S, S.lens + 288, 32, DB, 1, S.lut_d, S.cnt_d, S.sym_d, lane)) != ST_OK) return st;
                fixed = true;
            }
        } else {                                                      // dynamic codes
            fixed = false;
            if (r.pos() + 14 > end_bits) return ST_EXHAUSTED;
            r.refill();
            const int hlit = (int)r.take(5) + 257, hdist = (int)r.take(5) + 1, hclen = (int)r.take(4) + 4;
            if (hlit > 286 || hdist > 30) return ST_BAD_CODE;
            if (lane < 19) S.clens[lane] = 0;
            __syncthreads();
            for (int i = 0; i < hclen; i++) {
                r.refill();
                const uint32_t v = r.take(3);
                if (lane == 0) S.clens[S.order[i]] = (uint8_t)v;
            }
            __syncthreads();
            if ((st = build(S, S.clens, 19, CB, 2, S.lut_c, S.cnt_c, S.sym_c, lane)) != ST_OK) return st;
            const int total = hlit + hdist;
            for (int i = 0; i < total;) {
                if (r.pos() > end_bits) return ST_EXHAUSTED;
                const int sym = decode(r, S.lut_c, S.cnt_c, S.sym_c, CB);
                if (sym < 0) return ST_BAD_CODE;
                if (sym < 16) { if (lane == 0) S.lens[i] = (uint8_t)sym; i++; continue; }
                int val = 0, rep;
                if (sym == 16) {
                    if (i == 0) return ST_BAD_CODE;
                    __syncthreads();
                    val = S.lens[i - 1]; rep = 3 + (int)r.take(2);
                } else if (sym == 17) rep = 3 + (int)r.take(3);
                else rep = 11 + (int)r.take(7);
                if (i + rep > total) return ST_BAD_CODE;
                for (int j = lane; j < rep; j += 64) S.lens[i + j] = (uint8_t)val;
                i += rep;
            }
            __syncthreads();
            if (S.lens[256] == 0) return ST_BAD_CODE;                 // no end-of-block code
            if ((st = build(S, S.lens, hlit, LB, 0, S.lut_l, S.cnt_l, S.sym_l, lane)) != ST_OK) return st;
            if ((st = build(S, S.lens + hlit, hdist, DB, 1, S.lut_d, S.cnt_d, S.sym_d, lane)) != ST_OK) return st;
        }
        for (;;) {                                                    // every turn writes >= 1 byte of text or ends the block
            if (r.pos() > end_bits) return ST_EXHAUSTED;
            const int sym = decode(r, S.lut_l, S.cnt_l, S.sym_l, LB);
            if (sym < 0) return ST_BAD_SYMBOL;
            if (sym < 256) {
                if (pos >= M.isize) return ST_TOO_LONG;
                if (lane == 0) win[pos] = (uint8_t)sym;
                pos++;
                continue;
            }
            if (sym == 256) break;
            const int ls = sym - 257;
            if (ls >= 29) return ST_BAD_SYMBOL;
            const uint32_t len = S.lbase[ls] + r.take(S.lext[ls]);
            const int ds = decode(r, S.lut_d, S.cnt_d, S.sym_d, DB);
            if (ds < 0 || ds >= 30) return ST_BAD_SYMBOL;
            const uint32_t dist = S.dbase[ds] + r.take(S.dext[ds]);
            if (dist > pos) return ST_DISTANCE;
            if (pos + len > M.isize) return ST_TOO_LONG;
            __syncthreads();                                          // (the literals and matches in front are in the window)
            for (uint32_t j = (uint32_t)lane; j < len; j += 64) win[pos + j] = win[pos - dist + (dist >= len ? j : j % dist)];
            pos += len;
        }
    } while (!last);
    if (r.pos() > end_bits) return ST_EXHAUSTED;
    if ((r.pos() + 7) / 8 != pend) return ST_TRAILING;
    *out_pos = pos;
    if (pos != M.isize) return ST_TOO_SHORT;
    return ST_OK;
}

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap,
                                                    const DevMember *mem, uint32_t n, uint32_t *status) {
    __shared__ Lds S;
    const int lane = (int)threadIdx.x;
    const uint32_t m = blockIdx.x;
    if (m >= n) return;
    const DevMember M = mem[m];
    for (int i = lane; i < 256; i += 64) {
        uint32_t c = (uint32_t)i;
        for (int k = 0; k < 8; k++) c = (c & 1) ? (c >> 1) ^ POLY : c >> 1;
        S.crctab[i] = c;
    }
    if (lane < 32) S.x2n[lane] = c_x2n[lane];
    if (lane < 29) { S.lbase[lane] = c_lbase[lane]; S.lext[lane] = c_lext[lane]; }
    if (lane < 30) { S.dbase[lane] = c_dbase[lane]; S.dext[lane] = c_dext[lane]; }
    if (lane < 19) S.order[lane] = c_order[lane];
    __syncthreads();
    uint32_t st = ST_OK, got = 0;
    if (M.isize > MAX_ISIZE || M.in_len > in_bytes || M.in_off > in_bytes - M.in_len || M.isize > out_cap || M.out_off > out_cap - M.isize)
        st = ST_BAD_MEMBER;
    else
        st = inflate_member(S, M, in, in_bytes, &got, lane);
    __syncthreads();
    const uint32_t isize = M.isize;
    uint32_t word = st;
    if (st == ST_OK) {
        // CRC-32 of 64 slices (an odd number of dwords each: the lanes start in different LDS banks), combined
        uint32_t sl = ((isize + 63) / 64 + 3) & ~3u;
        if (((sl >> 2) & 1) == 0) sl += 4;
        const uint32_t a = std::min((uint32_t)lane * sl, isize), b = std::min(a + sl, isize);
        uint32_t c = 0xffffffffu;
        for (uint32_t i = a; i < b; i += 4) {
            const uint32_t w = S.win[i >> 2], k = std::min(4u, b - i);
            for (uint32_t q = 0; q < k; q++) c = S.crctab[(c ^ (w >> (8 * q))) & 255] ^ (c >> 8);
        }
        c ^= 0xffffffffu;
        const uint32_t xs = x2nmodp(sl, 3, S.x2n);
        uint32_t crc = 0;
        for (int i = 0; i < 64; i++) {
            const uint32_t ci = (uint32_t)__shfl((int)c, i);
            const uint32_t li = (uint32_t)__shfl((int)(b - a), i);
            if (li) crc = multmodp(li == sl ? xs : x2nmodp(li, 3, S.x2n), crc) ^ ci;
        }
        if (crc != M.crc) word = ST_CRC;
        // the text, coalesced: a head to the next 4-byte boundary of `out`, dwords, a tail
        const uint8_t *win = (const uint8_t *)S.win;
        uint8_t *o = out + M.out_off;
        const uint32_t head = std::min((uint32_t)((4u - (uint32_t)(M.out_off & 3)) & 3u), isize);
        if ((uint32_t)lane < head) o[lane] = win[lane];
        const uint32_t nw = (isize - head) / 4;
        uint32_t *o32 = (uint32_t *)(o + head);
        const uint32_t sh = (head & 3) * 8;
        for (uint32_t k = (uint32_t)lane; k < nw; k += 64) {
            const uint32_t wi = (head >> 2) + k;                     // (head < 4: the dwords of the window at head + 4k)
            const uint32_t lo = S.win[wi], hi = S.win[wi + 1];
            o32[k] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;
        }
        const uint32_t done = head + 4 * nw;
        if (done + (uint32_t)lane < isize) o[done + lane] = win[done + lane];
        if (isize) word |= ((uint32_t)win[isize - 1] << 8) | (1u << 16);
    }
    if (lane == 0) status[m] = word;
}

}  // namespace

hipError_t launch_inflate(hipStream_t s, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap,
                          const DevMember *mem, uint32_t n, uint32_t *status) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bgzf_inflate, dim3(n), dim3(64), 0, s, in, in_bytes, out, out_cap, mem, n, status);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// The device reader's buffers and the reader
// ------------------------------------------------------------------------------------------
namespace {
constexpr size_t IN_BATCH = 16u << 20;          // compressed bytes read per batch
constexpr size_t MAX_MEMBERS = 2048;            // members per batch (one workgroup each)
constexpr size_t OUT_CAP = MAX_MEMBERS * MAX_ISIZE;
}  // namespace

struct DevBufs {
    int device = 0;
    hipStream_t ks = nullptr, cs = nullptr;     // inflate kernels; text copies out of the batches
    struct Slot {
        uint8_t *h_in = nullptr, *d_in = nullptr, *d_out = nullptr;
        DevMember *h_mem = nullptr, *d_mem = nullptr;
        uint32_t *h_st = nullptr, *d_st = nullptr;
        hipEvent_t ev_done = nullptr, ev_free = nullptr;
        // the batch launched in the slot
        off_t pos = 0; size_t framed = 0, out_total = 0; bool eof = false;
        std::vector<Member> mem;
        std::vector<uint64_t> ends; std::vector<uint8_t> lasts;   // text end and last byte of each member with text
    } slot[2];
    std::vector<uint8_t *> text;                // device twins of the parser's pinned blocks
    std::vector<hipEvent_t> ev_text;
};

DevBufs *dev_bufs_new(int device, int n_blocks, size_t block, std::string &msg) {
    DevBufs *b = new DevBufs();
    b->device = device;
#define BG_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { msg = std::string(#call) + ": " + hipGetErrorString(e_); dev_bufs_free(b); return nullptr; } } while (0)
    BG_HIP(hipSetDevice(device));
    BG_HIP(hipStreamCreateWithFlags(&b->ks, hipStreamNonBlocking));
    BG_HIP(hipStreamCreateWithFlags(&b->cs, hipStreamNonBlocking));
    for (auto &s : b->slot) {
        BG_HIP(hipHostMalloc((void **)&s.h_in, IN_BATCH + 64, hipHostMallocDefault));
        BG_HIP(hipMalloc((void **)&s.d_in, IN_BATCH + 64));
        BG_HIP(hipMalloc((void **)&s.d_out, OUT_CAP + 64));
        BG_HIP(hipHostMalloc((void **)&s.h_mem, MAX_MEMBERS * sizeof(DevMember), hipHostMallocDefault));
        BG_HIP(hipMalloc((void **)&s.d_mem, MAX_MEMBERS * sizeof(DevMember)));
        BG_HIP(hipHostMalloc((void **)&s.h_st, MAX_MEMBERS * 4, hipHostMallocDefault));
        BG_HIP(hipMalloc((void **)&s.d_st, MAX_MEMBERS * 4));
        BG_HIP(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
        BG_HIP(hipEventCreateWithFlags(&s.ev_free, hipEventDisableTiming));
    }
    b->text.assign((size_t)n_blocks, nullptr);
    b->ev_text.assign((size_t)n_blocks, nullptr);
    for (auto &p : b->text) BG_HIP(hipMalloc((void **)&p, block + 64));
    for (auto &e : b->ev_text) BG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
#undef BG_HIP
    return b;
}

void dev_bufs_free(DevBufs *b) {
    if (!b) return;
    if (b->ks) hipStreamSynchronize(b->ks);
    if (b->cs) hipStreamSynchronize(b->cs);
    for (auto &s : b->slot) {
        if (s.h_in) hipHostFree(s.h_in);
        hipFree(s.d_in); hipFree(s.d_out); hipFree(s.d_mem); hipFree(s.d_st);
        if (s.h_mem) hipHostFree(s.h_mem);
        if (s.h_st) hipHostFree(s.h_st);
        if (s.ev_done) hipEventDestroy(s.ev_done);
        if (s.ev_free) hipEventDestroy(s.ev_free);
    }
    for (auto p : b->text) hipFree(p);
    for (auto e : b->ev_text) if (e) hipEventDestroy(e);
    if (b->ks) hipStreamDestroy(b->ks);
    if (b->cs) hipStreamDestroy(b->cs);
    delete b;
}

uint8_t *dev_bufs_block(DevBufs *b, int i) { return b->text[(size_t)i]; }
hipEvent_t dev_bufs_block_event(DevBufs *b, int i) { return b->ev_text[(size_t)i]; }
hipError_t dev_bufs_mark_block(DevBufs *b, int i) { return hipEventRecord(b->ev_text[(size_t)i], b->cs); }

bool DevReader::looks_like(int fd) {
    uint8_t h[64];
    const ssize_t m = ::pread(fd, h, sizeof h, 0);
    size_t hl;
    return m >= 18 && member_size(h, (size_t)m, &hl) != 0;
}

DevReader::DevReader(int fd, DevBufs *b, bool trace) : fd_(fd), b_(b), trace_(trace) { hipSetDevice(b->device); }

DevReader::~DevReader() {
    hipStreamSynchronize(b_->ks);                                     // (a batch launched ahead that nobody will read)
    hipStreamSynchronize(b_->cs);
    if (trace_) {
        if (hand_over_ >= 0)
            fprintf(stderr, "ingest trace: BGZF device reader, %llu members inflated on the GPU, then handed over to the sequential reader at byte %lld\n",
                    (unsigned long long)n_members_, (long long)hand_over_);
        else
            fprintf(stderr, "ingest trace: BGZF device reader, %llu members inflated on the GPU\n", (unsigned long long)n_members_);
    }
}

// the piece of the file at `pos` into slot s: frame its members and queue their inflation
bool DevReader::launch(int s, off_t pos, std::string &msg) {
    DevBufs::Slot &S = b_->slot[s];
    S.pos = pos; S.eof = false; S.framed = S.out_total = 0; S.mem.clear();
    size_t got = 0;
    while (got < IN_BATCH) {
        const ssize_t r = ::pread(fd_, S.h_in + got, IN_BATCH - got, pos + (off_t)got);
        if (r < 0) { if (errno == EINTR) continue; msg = std::string("read: ") + strerror(errno); return false; }
        if (r == 0) break;
        got += (size_t)r;
    }
    if (got == 0) { S.eof = true; return true; }
    S.framed = frame(S.h_in, got, S.mem, MAX_MEMBERS, OUT_CAP, &S.out_total);
    if (S.mem.empty()) return true;                                   // (the hand-over starts here)
    for (size_t i = 0; i < S.mem.size(); i++) {
        const Member &m = S.mem[i];
        S.h_mem[i] = DevMember{(uint64_t)m.in_off, (uint64_t)m.out_off, (uint32_t)m.in_len, m.isize, m.crc, 0};
    }
    const uint32_t n = (uint32_t)S.mem.size();
    hipError_t e = hipMemcpyAsync(S.d_in, S.h_in, (S.framed + 3) & ~(size_t)3, hipMemcpyHostToDevice, b_->ks);
    if (e == hipSuccess) e = hipMemcpyAsync(S.d_mem, S.h_mem, n * sizeof(DevMember), hipMemcpyHostToDevice, b_->ks);
    if (e == hipSuccess) e = hipStreamWaitEvent(b_->ks, S.ev_free, 0);     // (the text of the batch before in this slot has been copied out)
    if (e == hipSuccess) e = launch_inflate(b_->ks, S.d_in, S.framed, S.d_out, OUT_CAP, S.d_mem, n, S.d_st);
    if (e == hipSuccess) e = hipMemcpyAsync(S.h_st, S.d_st, n * 4, hipMemcpyDeviceToHost, b_->ks);
    if (e == hipSuccess) e = hipEventRecord(S.ev_done, b_->ks);
    if (e != hipSuccess) { msg = std::string("BGZF device inflate: ") + hipGetErrorString(e); return false; }
    return true;
}

// the batch of slot s is done: its good members become the text to deliver; the first bad one ends the reader's part
bool DevReader::settle(int s, std::string &msg) {
    DevBufs::Slot &S = b_->slot[s];
    cur_ = s; off_ = 0; text_len_ = 0;
    S.ends.clear(); S.lasts.clear();
    if (S.eof) { done_ = true; return true; }
    if (S.mem.empty()) { done_ = true; hand_over_ = S.pos; return true; }
    const hipError_t e = hipEventSynchronize(S.ev_done);
    if (e != hipSuccess) { msg = std::string("BGZF device inflate: ") + hipGetErrorString(e); return false; }
    size_t bad = S.mem.size();
    for (size_t i = 0; i < S.mem.size(); i++)
        if ((S.h_st[i] & 255u) != ST_OK) { bad = i; break; }
    for (size_t i = 0; i < bad; i++)
        if (S.h_st[i] & (1u << 16)) { S.ends.push_back(S.mem[i].out_off + S.mem[i].isize); S.lasts.push_back((uint8_t)(S.h_st[i] >> 8)); }
    n_members_ += bad;
    if (bad < S.mem.size()) {
        text_len_ = S.mem[bad].out_off;
        hand_over_ = S.pos + (off_t)S.mem[bad].hdr_off;
        if (bad > 0) any_ = true;
        done_ = true;
        return true;
    }
    text_len_ = S.out_total;
    any_ = true;
    pos_ = S.pos + (off_t)S.framed;
    return true;
}

long DevReader::read(uint8_t *dst, size_t cap, uint8_t *last, std::string &msg) {
    if (failed_) { msg = "BGZF device inflate: an earlier failure"; return -1; }
    for (;;) {
        if (cur_ >= 0) {
            DevBufs::Slot &S = b_->slot[cur_];
            if (off_ < text_len_ && cap > 0) {
                const size_t n = std::min(cap, text_len_ - off_);
                const hipError_t e = hipMemcpyAsync(dst, S.d_out + off_, n, hipMemcpyDeviceToDevice, b_->cs);
                if (e != hipSuccess) { failed_ = true; msg = std::string("BGZF device inflate: ") + hipGetErrorString(e); return -1; }
                off_ += n;
                const auto it = std::lower_bound(S.ends.begin(), S.ends.end(), (uint64_t)off_);
                if (it != S.ends.end() && *it == off_) *last = S.lasts[(size_t)(it - S.ends.begin())];
                if (off_ == text_len_) { hipEventRecord(S.ev_free, b_->cs); cur_ = -1; }
                return (long)n;
            }
            hipEventRecord(S.ev_free, b_->cs);
            cur_ = -1;
        }
        if (done_) return 0;
        int s = next_;
        if (s < 0) { s = 0; if (!launch(s, pos_, msg)) { failed_ = true; return -1; } }
        next_ = -1;
        if (!settle(s, msg)) { failed_ = true; return -1; }
        if (!done_) {                                                  // the next piece is read and inflated while this one is delivered
            if (!launch(s ^ 1, pos_, msg)) { failed_ = true; return -1; }
            next_ = s ^ 1;
        }
    }
}

}  // namespace bgzf
}  // namespace hulk

// ------------------------------------------------------------------------------------------
// hulk_bgzf_inflate: the kernel's own surface (whole members in a host buffer -> their text)
// ------------------------------------------------------------------------------------------
extern "C" int hulk_bgzf_inflate(const uint8_t *in, uint64_t in_len, uint8_t *out, uint64_t out_cap, uint64_t *out_len,
                                 uint64_t *n_members, uint64_t *bad_member, char *errbuf, uint64_t errbuf_len) {
    using namespace hulk::bgzf;
    std::string msg;
    int rc = HULK_OK;
    uint64_t total = 0, bad = UINT64_MAX;
    std::vector<Member> mem;
    auto finish = [&]() {
        if (out_len) *out_len = total;
        if (n_members) *n_members = mem.size();
        if (bad_member) *bad_member = bad;
        if (errbuf && errbuf_len) {
            const size_t k = std::min<size_t>(msg.size(), (size_t)errbuf_len - 1);
            memcpy(errbuf, msg.data(), k); errbuf[k] = 0;
        }
        return rc;
    };
    if (!in && in_len) { rc = HULK_ERR_ARG; msg = "hulk_bgzf_inflate: NULL input"; return finish(); }
    size_t out_total = 0;
    const size_t framed = in_len ? frame(in, (size_t)in_len, mem, SIZE_MAX, SIZE_MAX, &out_total) : 0;
    total = out_total;
    if (framed != in_len) {
        bad = mem.size();
        rc = HULK_ERR_IO;
        msg = "bgzf: member " + std::to_string(bad) + " (byte " + std::to_string(framed) + "): not a whole BGZF member";
        return finish();
    }
    if (!out) return finish();                                        // (the size query)
    if (out_cap < total) { rc = HULK_ERR_ARG; msg = "hulk_bgzf_inflate: out_cap is smaller than the text"; return finish(); }
    if (mem.empty()) return finish();
    uint8_t *d_in = nullptr, *d_out = nullptr;
    DevMember *d_mem = nullptr;
    uint32_t *d_st = nullptr;
    std::vector<DevMember> h_mem(mem.size());
    std::vector<uint32_t> h_st(mem.size());
    for (size_t i = 0; i < mem.size(); i++)
        h_mem[i] = DevMember{(uint64_t)mem[i].in_off, (uint64_t)mem[i].out_off, (uint32_t)mem[i].in_len, mem[i].isize, mem[i].crc, 0};
    hipError_t e = hipMalloc((void **)&d_in, in_len + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&d_out, total + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&d_mem, mem.size() * sizeof(DevMember));
    if (e == hipSuccess) e = hipMalloc((void **)&d_st, mem.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_in, in, in_len, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_mem, h_mem.data(), mem.size() * sizeof(DevMember), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_inflate(nullptr, d_in, in_len, d_out, total, d_mem, (uint32_t)mem.size(), d_st);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(h_st.data(), d_st, mem.size() * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total) e = hipMemcpy(out, d_out, total, hipMemcpyDeviceToHost);
    hipFree(d_in); hipFree(d_out); hipFree(d_mem); hipFree(d_st);
    if (e != hipSuccess) { rc = HULK_ERR_HIP; msg = std::string("hulk_bgzf_inflate: ") + hipGetErrorString(e); return finish(); }
    for (size_t i = 0; i < mem.size(); i++)
        if ((h_st[i] & 255u) != ST_OK) {
            bad = i; rc = HULK_ERR_IO;
            msg = "bgzf: member " + std::to_string(i) + " (byte " + std::to_string(mem[i].hdr_off) + "): " + status_text(h_st[i] & 255u);
            break;
        }
    return finish();
}
