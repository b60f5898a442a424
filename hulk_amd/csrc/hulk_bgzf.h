// hulk_bgzf.h — BGZF (bgzip / htslib) members: the framing the host readers share, and the device inflater of hulk_bgzf.hip
// (k_bgzf_inflate and DevReader, the reader HULK_INGEST_DEVICE_INFLATE puts in front of the device parsers).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <sys/types.h>

#include <string>
#include <vector>

namespace hulk {
namespace bgzf {

constexpr size_t MAX_ISIZE = 1u << 16;     // text of one member (bgzip writes at most 65,280 bytes)

// total size of the member whose header starts at p (n bytes available), 0 = not a BGZF member / header incomplete
inline size_t member_size(const uint8_t *p, size_t n, size_t *header_len) {
    if (n < 18 || p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || p[3] != 4) return 0;       // FEXTRA and nothing else
    const size_t xlen = (size_t)p[10] | ((size_t)p[11] << 8);
    if (n < 12 + xlen) return 0;
    size_t bsize = 0; bool found = false;
    for (size_t o = 12; o + 4 <= 12 + xlen;) {
        const size_t sl = (size_t)p[o + 2] | ((size_t)p[o + 3] << 8);
        if (o + 4 + sl > 12 + xlen) return 0;
        if (p[o] == 'B' && p[o + 1] == 'C' && sl == 2 && !found) { bsize = (size_t)p[o + 4] | ((size_t)p[o + 5] << 8); found = true; }
        o += 4 + sl;
    }
    if (!found) return 0;
    const size_t total = bsize + 1;
    if (total < 12 + xlen + 2 + 8) return 0;                   // header + the shortest deflate stream + trailer
    *header_len = 12 + xlen;
    return total;
}

// one member of a piece of the file: header at hdr_off, deflate payload [in_off, in_off + in_len), text at out_off (the
// ISIZEs of the members in front of it, summed), the trailer's CRC-32 and ISIZE
struct Member { size_t hdr_off, in_off, in_len, out_off; uint32_t crc, isize; };

// The whole members that lie in p[0..n), appended to `mem` (cleared first): framing stops at the first thing that is not a
// whole BGZF member of at most MAX_ISIZE bytes of text, or where one more member would pass `max_members` or `max_out`
// bytes of text.  Returns the bytes framed; *out_total = their text.
inline size_t frame(const uint8_t *p, size_t n, std::vector<Member> &mem, size_t max_members, size_t max_out, size_t *out_total) {
    mem.clear();
    size_t o = 0, out = 0;
    while (o < n && mem.size() < max_members) {
        size_t hl = 0;
        const size_t total = member_size(p + o, n - o, &hl);
        if (total == 0 || o + total > n) break;
        Member m;
        m.hdr_off = o; m.in_off = o + hl; m.in_len = total - hl - 8; m.out_off = out;
        const uint8_t *t = p + o + total - 8;
        m.crc = (uint32_t)t[0] | ((uint32_t)t[1] << 8) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 24);
        m.isize = (uint32_t)t[4] | ((uint32_t)t[5] << 8) | ((uint32_t)t[6] << 16) | ((uint32_t)t[7] << 24);
        if (m.isize > MAX_ISIZE || out + m.isize > max_out) break;
        mem.push_back(m);
        out += m.isize; o += total;
    }
    *out_total = out;
    return o;
}

// ---- device side ----------------------------------------------------------------------------------------------------
// per-member result of k_bgzf_inflate: status in bits 0..7 (ST_*), the member's last text byte in bits 8..15, bit 16 set
// when the member has text
enum : uint32_t {
    ST_OK = 0, ST_BLOCK_TYPE, ST_BAD_CODE, ST_BAD_SYMBOL, ST_DISTANCE, ST_TOO_LONG, ST_TOO_SHORT, ST_EXHAUSTED, ST_TRAILING,
    ST_CRC, ST_STORED_LEN, ST_BAD_MEMBER, ST_COUNT
};
const char *status_text(uint32_t st);

struct DevMember { uint64_t in_off, out_off; uint32_t in_len, isize, crc, pad; };

// members [0, n) of `in` (in_bytes bytes, 4-byte aligned, readable up to in_bytes rounded up to 4) into `out` (out_cap bytes)
hipError_t launch_inflate(hipStream_t s, const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap,
                          const DevMember *mem, uint32_t n, uint32_t *status);

// The buffers of the device reader, one set per device-parser buffer set (FqDev): two batches of members (pinned and device
// compressed bytes, device text, member tables, status records) and a device twin of each of the parser's pinned blocks —
// the reader thread places device text there, the parser's copy stream takes it on to the raw block.
struct DevBufs;
DevBufs *dev_bufs_new(int device, int n_blocks, size_t block, std::string &msg);
void dev_bufs_free(DevBufs *b);
uint8_t *dev_bufs_block(DevBufs *b, int i);           // device twin of pinned block i
hipEvent_t dev_bufs_block_event(DevBufs *b, int i);   // recorded behind the copies into twin i (dev_bufs_mark_block)
hipError_t dev_bufs_mark_block(DevBufs *b, int i);

// One regular file whose first member is BGZF, inflated on the device batch by batch (GzBgzf's rule: at the first member that is
// anything but a clean, verified BGZF member, the text in front of it is delivered and the file is handed over at that member).
class DevReader {
 public:
    static bool looks_like(int fd);
    DevReader(int fd, DevBufs *b, bool trace);
    ~DevReader();
    // Up to cap bytes of text copied (asynchronously, on the buffers' copy stream) to device memory at dst; *last = the last of
    // them when they end a member.  0: the file's members are over — hand_over() >= 0: the rest of the file, from that offset, is
    // the sequential reader's (any_member(): members were read before it).  -1: a HIP failure (msg).
    long read(uint8_t *dst, size_t cap, uint8_t *last, std::string &msg);
    off_t hand_over() const { return hand_over_; }
    bool any_member() const { return any_; }

 private:
    bool launch(int slot, off_t pos, std::string &msg);
    bool settle(int slot, std::string &msg);
    int fd_;
    DevBufs *b_;
    bool trace_;
    int cur_ = -1, next_ = -1;            // slot whose text is delivered; slot launched behind it
    size_t off_ = 0, text_len_ = 0;
    off_t pos_ = 0, hand_over_ = -1;
    bool done_ = false, any_ = false, failed_ = false;
    uint64_t n_members_ = 0;
};

}  // namespace bgzf
}  // namespace hulk
