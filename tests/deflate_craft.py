"""A DEFLATE (RFC 1951) encoder for tests: valid streams of the shapes zlib's encoder never writes, and malformed ones.

There is no match finder: a text is what a list of tokens expands to, ("lit", byte) and ("match", length, distance), and a block
is written from its tokens with whatever code lengths the caller gives it — codes of up to 15 bits on everyday symbols, full
alphabets, a lone distance code or none, a code-length code of 7 bits, repeat codes that run from the literal/length lengths
into the distance lengths, blocks joined at bit boundaries.  Every valid stream handed out (Stream.finish) has been inflated by
zlib.decompressobj(-15): the result must be the expanded text, with `eof` set and nothing left over — a failure there is a bug
in this file and raises.  The corpus functions at the end are seeded and deterministic; tests/test_deflate_crafted_cpu.py runs
them through the host decoders, tests/test_gpu_bgzf_crafted.py through k_bgzf_inflate, tools/fuzz_bgzf_device.py --crafted
through the device reader."""
import random
import struct
import zlib

LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
EOB = 256


# ------------------------------------------------------------------------------------------------------------------------------
# bits and codes
# ------------------------------------------------------------------------------------------------------------------------------
class BitWriter:
    """LSB-first bit stream; whole bytes leave the accumulator as they fill"""
    __slots__ = ("out", "acc", "n")

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def bits(self, value, count):
        self.acc |= value << self.n
        self.n += count
        if self.n >= 8:
            k = self.n >> 3
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n &= 7

    def code(self, c):                              # c = (bits of the code already reversed, length): canonical_codes()
        self.bits(c[0], c[1])

    def align(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0

    def raw(self, data):
        assert self.n == 0
        self.out += data

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc & 255]) if self.n else b"")


def canonical_codes(lengths):
    """code of every symbol as (code reversed for LSB-first writing, length), None for length 0; the set need not be complete"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 17, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
            continue
        c = nxt[l] & ((1 << l) - 1)
        nxt[l] += 1
        out.append((int(format(c, "0%db" % l)[::-1], 2), l))
    return out


def kraft(lengths, maxbits=15):
    """sum of 2^(maxbits - l): == 2^maxbits for a complete set, more when over-subscribed"""
    return sum(1 << (maxbits - l) for l in lengths if l)


FIXED_LL_LENGTHS = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_LL = canonical_codes(FIXED_LL_LENGTHS)
FIXED_D = canonical_codes([5] * 32)


def len_symbol(n):
    """(symbol, extra bits, extra value) of match length n"""
    assert 3 <= n <= 258
    i = max(k for k in range(29) if LEN_BASE[k] <= n)
    return 257 + i, LEN_EXTRA[i], n - LEN_BASE[i]


_LEN_SYM = [None] * 3 + [len_symbol(n) for n in range(3, 259)]
_DIST_SYM = [None] + [(i, DIST_EXTRA[i], x) for i in range(30) for x in range(1 << DIST_EXTRA[i])]


def dist_symbol(d):
    """(symbol, extra bits, extra value) of match distance d"""
    assert 1 <= d <= 32768
    return _DIST_SYM[d]


# ------------------------------------------------------------------------------------------------------------------------------
# tokens
# ------------------------------------------------------------------------------------------------------------------------------
def lits(data):
    return [("lit", b) for b in data]


def extend(text, tokens):
    """append what `tokens` expand to, to the bytearray `text`"""
    for t in tokens:
        if t[0] == "lit":
            text.append(t[1])
        else:
            _, n, d = t
            assert 3 <= n <= 258 and 1 <= d <= min(32768, len(text)), (t, len(text))
            at = len(text) - d
            if d >= n:
                text += text[at:at + n]
            else:
                seg = bytes(text[at:])
                text += (seg * (n // d + 1))[:n]
    return text


def expand(tokens, text_so_far=b""):
    """the text: `text_so_far` and what the tokens add to it"""
    return bytes(extend(bytearray(text_so_far), tokens))


def used_symbols(tokens):
    """(literal/length symbols, distance symbols) the tokens need — the end-of-block code included"""
    ll, dd = {EOB}, set()
    for t in tokens:
        if t[0] == "lit":
            ll.add(t[1])
        else:
            ll.add(_LEN_SYM[t[1]][0])
            dd.add(dist_symbol(t[2])[0])
    return ll, dd


# ------------------------------------------------------------------------------------------------------------------------------
# code shapes: complete sets of n code lengths, sorted ascending
# ------------------------------------------------------------------------------------------------------------------------------
def balanced_lengths(n):
    if n == 1:
        return [1]
    b = n.bit_length() - 1
    lo = (1 << (b + 1)) - n
    return [b] * lo + [b + 1] * (n - lo)


def deepest_lengths(n, maxbits=15):
    """as deep as it goes: 1, 2, 3, ..., k and the other n - k balanced under the last node, for the largest k that keeps every
    code within maxbits (n <= 16: 1, 2, ..., n - 1, n - 1)"""
    assert 2 <= n <= 1 << maxbits
    for k in range(min(n - 2, maxbits - 1), -1, -1):
        rest = balanced_lengths(n - k)
        if k + rest[-1] <= maxbits:
            return list(range(1, k + 1)) + [k + l for l in rest]
    raise AssertionError


def random_lengths(n, rng, maxbits=15, chain=0.5):
    """random leaf splitting: n - 1 times a leaf above maxbits becomes two; `chain` = how often the newest leaf is the one split
    (1.0 gives the deepest shape, 0.0 bushy ones)"""
    assert 2 <= n <= 1 << maxbits
    open_, closed = [0], []
    for _ in range(n - 1):
        i = len(open_) - 1 if rng.random() < chain else rng.randrange(len(open_))
        open_[i], open_[-1] = open_[-1], open_[i]
        d = open_.pop() + 1
        (open_ if d < maxbits else closed).extend((d, d))
    return sorted(open_ + closed)


def assign(sorted_lengths, symbols, size, rng=None, long_for=()):
    """lengths list of `size` entries: `symbols` get `sorted_lengths` in a random order, those in `long_for` the longest"""
    symbols = list(symbols)
    assert len(symbols) == len(sorted_lengths) and max(symbols) < size
    first = [s for s in symbols if s not in long_for]
    last = [s for s in symbols if s in long_for]
    if rng is not None:
        rng.shuffle(first)
        rng.shuffle(last)
    out = [0] * size
    for s, l in zip(first + last, sorted_lengths):
        out[s] = l
    return out


def make_codes(tokens, rng, shape="deepest", pad_ll=(), pad_d=(), full=False, trim=True, lone=True, long_used=True):
    """(litlen_lengths, dist_lengths) for a block of `tokens`.  The used symbols get a code, with those of pad_ll / pad_d (full:
    all 286 / 30).  shape: "deepest", "random" or "balanced".  trim: the lists end at the last symbol with a code (the minimum
    HLIT / HDIST), else they have 286 / 30 entries.  One used distance symbol gets the lone 1-bit code when `lone` (else a
    second symbol makes the set complete); no match at all gives HDIST = 1 with length 0.  long_used: the used symbols get the
    longest codes of the set, the padding the short ones."""
    ll_used, d_used = used_symbols(tokens)
    ll_syms = set(ll_used) | set(pad_ll) | (set(range(286)) if full else set())
    d_syms = set(d_used) | set(pad_d) | (set(range(30)) if full else set())
    if len(ll_syms) == 1:
        ll_syms.add(ord("A") if ord("A") not in ll_syms else ord("C"))
    if len(d_syms) == 1 and not lone:
        d_syms.add(0 if 0 not in d_syms else 1)

    def shaped(n, maxbits=15):
        if shape == "deepest":
            return deepest_lengths(n, maxbits)
        if shape == "balanced":
            return balanced_lengths(n)
        return random_lengths(n, rng, maxbits, rng.choice((0.0, 0.3, 0.7, 0.9, 1.0)))
    ll = assign(shaped(len(ll_syms)), sorted(ll_syms), max(ll_syms) + 1 if trim else 286, rng, ll_used if long_used else ())
    ll += [0] * (257 - len(ll))
    if not d_syms:
        dl = [0] if trim else [0] * 30
    elif len(d_syms) == 1:
        s = min(d_syms)
        dl = [0] * (s + 1 if trim else 30)
        dl[s] = 1
    else:
        dl = assign(shaped(len(d_syms)), sorted(d_syms), max(d_syms) + 1 if trim else 30, rng, d_used if long_used else ())
    return ll, dl


# ------------------------------------------------------------------------------------------------------------------------------
# blocks (appended to a BitWriter at whatever bit it stands)
# ------------------------------------------------------------------------------------------------------------------------------
def stored_block(w, data, last=False):
    assert len(data) <= 65535
    w.bits(1 if last else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack("<HH", len(data), len(data) ^ 0xffff))
    w.raw(data)


def put_tokens(w, tokens, llc, dc, eob=True):
    for t in tokens:
        if t[0] == "lit":
            w.code(llc[t[1]])
        else:
            s, xb, xv = _LEN_SYM[t[1]]
            w.code(llc[s])
            if xb:
                w.bits(xv, xb)
            s, xb, xv = dist_symbol(t[2])
            w.code(dc[s])
            if xb:
                w.bits(xv, xb)
    if eob:
        w.code(llc[EOB])


def fixed_block(w, tokens, last=False):
    w.bits(1 if last else 0, 1)
    w.bits(1, 2)
    put_tokens(w, tokens, FIXED_LL, FIXED_D)


def rle_ops(seq, rng=None):
    """a sequence of code lengths as code-length symbols (symbol, extra bits, extra value), runs coded with 16 / 17 / 18"""
    ops, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if rng is not None and rng.random() < 0.15:
            run = 1                                                        # (now and then a run is left alone)
        if v == 0 and run >= 3:
            r = min(run, 138)
            if rng is not None:
                r = rng.randint(3, r)
            ops.append((17, 3, r - 3) if r <= 10 else (18, 7, r - 11))
            i += r
        elif v != 0 and run >= 4:
            ops.append((v, 0, 0))
            i, left = i + 1, run - 1
            while left >= 3:
                r = min(left, 6)
                if rng is not None:
                    r = rng.randint(3, r)
                ops.append((16, 2, r - 3))
                i, left = i + r, left - r
        else:
            ops.append((v, 0, 0))
            i += 1
    return ops


def ops_lengths(ops):
    """what a decoder makes of the code-length symbols"""
    out = []
    for s, _, xv in ops:
        if s < 16:
            out.append(s)
        elif s == 16:
            out += [out[-1]] * (3 + xv)
        else:
            out += [0] * ((3 if s == 17 else 11) + xv)
    return out


def dynamic_header(w, ll, dl, last=False, rle=True, cross=True, hclen19=False, deep_clc=False, rng=None, ops=None, clc=None,
                   hlit=None, hdist=None):
    """BFINAL, BTYPE = 2 and the code lengths.  rle: runs coded with 16 / 17 / 18 (cross: over the literal/length and distance
    lengths as one sequence, so that a run may go from the one into the other) or every length on its own; hclen19: all 19
    code-length code lengths are sent, else they end at the last one in use; deep_clc: the code-length code is as deep as 7
    bits goes, else balanced.  ops / clc / hlit / hdist override what is written (malformed headers).  Returns
    {"cross": a repeat ran from the literal/length into the distance lengths, "clc_max": longest code-length code}."""
    if ops is None:
        if not rle:
            ops = [(v, 0, 0) for v in ll + dl]
        elif cross:
            ops = rle_ops(ll + dl, rng)
        else:
            ops = rle_ops(ll, rng) + rle_ops(dl, rng)
    if clc is None:
        used = sorted({s for s, _, _ in ops})
        while len(used) < 2:                                               # (a lone code-length code is not allowed)
            used = sorted(set(used) | {min(s for s in range(19) if s not in used)})
        shape = deepest_lengths(len(used), 7) if deep_clc else balanced_lengths(len(used))
        clc = assign(shape, used, 19, rng)
    hclen = 19 if hclen19 else max(4, max(i for i in range(19) if clc[CL_ORDER[i]]) + 1)
    w.bits(1 if last else 0, 1)
    w.bits(2, 2)
    w.bits(len(ll) - 257 if hlit is None else hlit, 5)
    w.bits(len(dl) - 1 if hdist is None else hdist, 5)
    w.bits(hclen - 4, 4)
    for i in range(hclen):
        w.bits(clc[CL_ORDER[i]], 3)
    cc = canonical_codes(clc)
    at, crossed = 0, False
    for s, xb, xv in ops:
        w.code(cc[s])
        if xb:
            w.bits(xv, xb)
        n = 1 if s < 16 else (3 if s in (16, 17) else 11) + xv
        crossed |= s >= 16 and at < len(ll) < at + n
        at += n
    return {"cross": crossed, "clc_max": max(clc)}


def dynamic_block(w, tokens, litlen_lengths, dist_lengths, last=False, **header):
    info = dynamic_header(w, litlen_lengths, dist_lengths, last, **header)
    put_tokens(w, tokens, canonical_codes(litlen_lengths), canonical_codes(dist_lengths))
    return info


class Stream:
    """one raw DEFLATE stream under construction: blocks appended at bit boundaries, the text they expand to kept beside"""

    def __init__(self, name=""):
        self.name, self.w, self.text = name, BitWriter(), bytearray()
        self.done = False
        # what the stream reaches: the longest literal/length and distance codes USED, blocks with a lone distance code / with
        # none, repeats that crossed from literal/length into distance lengths, the longest code-length code, blocks
        self.info = {"ll_max": 0, "d_max": 0, "lone": 0, "nodist": 0, "cross": 0, "clc_max": 0, "blocks": 0, "hlit_max": 0, "hdist_max": 0}

    def _end(self, last):
        assert not self.done
        self.done = last
        self.info["blocks"] += 1
        return self

    def stored(self, data, last=False):
        stored_block(self.w, data, last)
        self.text += data
        return self._end(last)

    def fixed(self, tokens, last=False):
        fixed_block(self.w, tokens, last)
        extend(self.text, tokens)
        return self._end(last)

    def dynamic(self, tokens, ll, dl, last=False, **header):
        assert 257 <= len(ll) <= 286 and 1 <= len(dl) <= 30
        assert kraft(ll) == 1 << 15, "literal/length set"
        nd = sum(1 for l in dl if l)
        assert nd == 0 or (nd == 1 and max(dl) == 1) or kraft(dl) == 1 << 15, "distance set"
        ll_used, d_used = used_symbols(tokens)
        h = dynamic_block(self.w, tokens, ll, dl, last, **header)
        extend(self.text, tokens)
        i = self.info
        i["ll_max"] = max(i["ll_max"], max(ll[s] for s in ll_used))
        i["d_max"] = max([i["d_max"]] + [dl[s] for s in d_used])
        i["lone"] += nd == 1
        i["nodist"] += nd == 0
        i["cross"] += h["cross"]
        i["clc_max"] = max(i["clc_max"], h["clc_max"])
        i["hlit_max"], i["hdist_max"] = max(i["hlit_max"], len(ll)), max(i["hdist_max"], len(dl))
        return self._end(last)

    def finish(self):
        """(deflate stream, text) — checked: zlib inflates the one to the other, ends there and leaves nothing over"""
        assert self.done, "no final block"
        body, text = self.w.getvalue(), bytes(self.text)
        z = zlib.decompressobj(-15)
        got = z.decompress(body)
        if got != text or not z.eof or z.unused_data:
            raise AssertionError("deflate_craft: zlib disagrees on stream %r (eof %r, %d bytes left over, %d of %d bytes of text)"
                                 % (self.name, z.eof, len(z.unused_data), len(got), len(text)))
        return body, text


# ------------------------------------------------------------------------------------------------------------------------------
# containers
# ------------------------------------------------------------------------------------------------------------------------------
def bgzf_member(text, body):
    """one BGZF member: gzip header with the BC subfield, the raw deflate `body`, CRC-32 and ISIZE of `text`"""
    total = 12 + 6 + len(body) + 8
    assert total <= 65536 and len(body) >= 2, total
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + (total - 1).to_bytes(2, "little") + body
            + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff))


def gzip_member(text, body):
    return b"\x1f\x8b\x08\0\0\0\0\0\0\xff" + body + struct.pack("<II", zlib.crc32(text) & 0xffffffff, len(text) & 0xffffffff)


def zlib_verdict(body):
    """("accept", text) when zlib inflates the raw stream to its end, ("reject", None) when it refuses it or wants more"""
    z = zlib.decompressobj(-15)
    try:
        got = z.decompress(body)
    except zlib.error:
        return "reject", None
    return ("accept", got) if z.eof else ("reject", None)


# ------------------------------------------------------------------------------------------------------------------------------
# FASTQ from tokens
# ------------------------------------------------------------------------------------------------------------------------------
TEXT_BYTES = tuple(b for b in range(256) if b in (9, 10, 13) or 32 <= b <= 126)


class FastqTokens:
    """records as tokens, every one valid FASTQ: a header of literals, a sequence of literals or a match copying an earlier read
    (which must lie within `text`, the inflated text of the member so far, at most 32 KiB back), `+`, and a quality line that is
    one literal and a distance-1 match, or literals"""

    def __init__(self, rng, lo=60, hi=250):
        self.rng, self.lo, self.hi, self.n = rng, lo, hi, 0
        self.reads = []                                                    # (offset in the member's text, length) of earlier sequences

    def new_member(self):
        self.reads = []

    def record(self, text):
        rng = self.rng
        L = rng.randint(self.lo, self.hi)
        toks = lits(b"@r%d\n" % self.n)
        self.n += 1
        at = len(text) + len(toks)
        self.reads = [r for r in self.reads if at + L - r[0] <= 32768]
        src = [r for r in self.reads if r[1] >= L]
        if src and rng.random() < 0.6:
            o, _ = rng.choice(src)
            left = L
            while left:                                                    # (<= 258 bytes: one match, now and then two)
                n = left if left <= 258 and (left < 6 or rng.random() < 0.7) else rng.randint(3, min(258, left - 3))
                toks.append(("match", n, at - o))
                left -= n
        else:
            toks += lits(bytes(rng.choice(b"ACGT") for _ in range(L)))
        self.reads.append((at, L))
        toks += lits(b"\n+\n")
        if rng.random() < 0.6 and L >= 4:
            toks += [("lit", rng.choice(b"FI:,#")), ("match", L - 1, 1)] if L - 1 <= 258 else lits(b"F" * L)
        else:
            toks += lits(bytes(rng.choice(b"FFFFFFF:,F#") for _ in range(L)))
        toks.append(("lit", 10))
        return toks


def blocks_of(stream, tokens, rng, lo=20, hi=400, pad_text=False, last=True, kinds=("dynamic",)):
    """`tokens` as a chain of small blocks with random code shapes and header choices, appended to `stream`"""
    at = 0
    while True:
        n = rng.randint(lo, hi)
        part, at = tokens[at:at + n], at + n
        end = last and at >= len(tokens)
        kind = rng.choice(kinds)
        if kind == "fixed":
            stream.fixed(part, end)
        elif kind == "stored":
            stream.stored(expand(part, stream.text)[len(stream.text):], end)
        else:
            pad = [s for s in rng.sample(TEXT_BYTES, rng.randint(0, 40))] + list(range(257, rng.choice((257, 270, 286)))) if pad_text else ()
            ll, dl = make_codes(part, rng, rng.choice(("deepest", "deepest", "random")), pad_ll=pad, pad_d=range(rng.choice((0, 0, 12, 30))),
                                trim=rng.random() < 0.7, lone=rng.random() < 0.7)
            stream.dynamic(part, ll, dl, end, rle=rng.random() < 0.8, cross=rng.random() < 0.8, hclen19=rng.random() < 0.3,
                           deep_clc=rng.random() < 0.5, rng=rng)
        if at >= len(tokens):
            return stream


def fastq_gzip(seed, size):
    """(file bytes, sequences, info): ONE gzip member of about `size` bytes of FASTQ, many small dynamic blocks of deep codes"""
    rng = random.Random(seed)
    fq, st = FastqTokens(rng), Stream("fastq_gzip %d" % seed)
    while len(st.text) < size:
        toks = []
        shadow = bytearray(st.text[-33000:])
        base = len(st.text) - len(shadow)
        fq.reads = [(o - base, n) for o, n in fq.reads if o >= base]
        for _ in range(rng.randint(1, 6)):
            rec = fq.record(shadow)
            extend(shadow, rec)
            toks += rec
        fq.reads = [(o + base, n) for o, n in fq.reads]
        del fq.reads[:-200]
        blocks_of(st, toks, rng, pad_text=True, last=False)
    st.stored(b"", True)
    body, text = st.finish()
    lines = text.split(b"\n")
    return gzip_member(text, body), lines[1::4], dict(st.info, text=len(text))


def fastq_bgzf(seed, size, lo=300, hi=65280, bad_member=None):
    """(file bytes, sequences, info) of fastq_bgzf_members"""
    members, seqs, info = fastq_bgzf_members(seed, size, lo, hi, bad_member)
    return b"".join(members), seqs, info


def fastq_bgzf_members(seed, size, lo=300, hi=65280, bad_member=None):
    """(members, sequences, info): a BGZF file of about `size` bytes of FASTQ in members of random sizes (records straddle
    them), each a chain of small dynamic blocks of deep codes, and the empty end-of-file member.  bad_member = (index, body,
    text): that member is replaced by a malformed one."""
    rng = random.Random(seed)
    fq = FastqTokens(rng)
    out, total, info = [], 0, {"ll_max": 0, "d_max": 0, "lone": 0, "nodist": 0, "members": 0}
    state = {"toks": [], "text": bytearray(), "target": rng.randint(lo, hi)}
    whole = bytearray()

    def close():
        st = Stream("fastq_bgzf %d member %d" % (seed, len(out)))
        if state["toks"]:
            blocks_of(st, state["toks"], rng, hi=2000)
        else:
            st.fixed([], True)
        body, text = st.finish()
        while 26 + len(body) > 65536:                                      # (deep codes on literals only: too big — stored then)
            st = Stream().stored(text[:65535], len(text) <= 65535)
            if len(text) > 65535:
                st.stored(text[65535:], True)
            body, text = st.finish()
        for k in ("ll_max", "d_max"):
            info[k] = max(info[k], st.info[k])
        info["lone"] += st.info["lone"]; info["nodist"] += st.info["nodist"]; info["members"] += 1
        if bad_member is not None and len(out) == bad_member[0]:
            out.append(bgzf_member(bad_member[2], bad_member[1]))
        else:
            out.append(bgzf_member(text, body))
        state["toks"], state["text"], state["target"] = [], bytearray(), rng.randint(lo, hi)
        fq.new_member()

    while len(whole) < size:
        rec = fq.record(state["text"])
        data = expand(rec, state["text"])[len(state["text"]):]
        whole += data
        off = 0
        for i, t in enumerate(rec):
            n = 1 if t[0] == "lit" else t[1]
            if len(state["text"]) + n > state["target"] and state["toks"]:
                close()                                                     # the rest of the record opens the next member, as literals
                state["toks"] = lits(data[off:])
                state["text"] += data[off:]
                break
            state["toks"].append(t)
            extend(state["text"], (t,))
            off += n
    close()
    out.append(bgzf_member(b"", Stream().fixed([], True).finish()[0]))
    return out, bytes(whole).split(b"\n")[1::4], info


# ------------------------------------------------------------------------------------------------------------------------------
# the corpus
# ------------------------------------------------------------------------------------------------------------------------------
# how a planned token list becomes streams: fixed codes, deepest dynamic codes with plain and with run-length headers, and a
# 7-bit code-length code with all 19 of its lengths sent
ENCODINGS = ("fixed", "deep-plain", "deep-rle", "clc7")


def encode(name, blocks, how, rng, **codes):
    """one valid stream from a list of token lists (one block each)"""
    st = Stream("%s/%s" % (name, how))
    for i, toks in enumerate(blocks):
        last = i == len(blocks) - 1
        if how == "fixed":
            st.fixed(toks, last)
        else:
            ll, dl = make_codes(toks, rng, "deepest", **codes)
            st.dynamic(toks, ll, dl, last, rle=how != "deep-plain", hclen19=how == "clc7", deep_clc=how == "clc7", rng=None)
    body, text = st.finish()
    return {"name": st.name, "body": body, "text": text, "info": st.info}


def _filler(rng, n):
    return lits(bytes(rng.choice(b"ACGTN\n@+FI:") for _ in range(n)))


def planned_token_lists(seed=1):
    """[(name, [block token lists], make_codes arguments)]: the planned valid cases, every text at most 65,536 bytes"""
    rng = random.Random(seed)
    out = []
    # every length symbol at the lowest and highest value of its extra bits
    toks = _filler(rng, 300)
    for i in range(29):
        for n in sorted({LEN_BASE[i], LEN_BASE[i] + (1 << LEN_EXTRA[i]) - 1}):
            toks += [("match", n, rng.choice((1, 2, 7, 64, 300))), ("lit", rng.choice(b"ACGT"))]
    out.append(("length symbols", [toks], {}))
    # every distance symbol at both ends, up to 32,768: the text grows by 258-byte matches
    toks = _filler(rng, 258)
    size, k = 258, 0
    for i in range(30):
        for d in sorted({DIST_BASE[i], DIST_BASE[i] + (1 << DIST_EXTRA[i]) - 1}):
            while size < d:
                toks.append(("match", 258, 258)); size += 258
            n = (3, 4, 64, 65, 258)[k % 5]; k += 1
            toks += [("match", n, d), ("lit", rng.choice(b"ACGT"))]; size += n + 1
    out.append(("distance symbols", [toks], {}))
    # overlapping copies
    lens = lambda d: sorted({n for n in (3, 4, d, d + 1, 63, 64, 65, 127, 128, 129, 257, 258) if 3 <= n <= 258})
    for name, ds in (("overlap 1-35", range(1, 36)), ("overlap 36-70", range(36, 71)), ("overlap 127-257", (127, 128, 129, 255, 256, 257))):
        toks = lits(bytes(rng.randrange(33, 127) for _ in range(260)))
        for d in ds:
            for n in lens(d):
                toks += [("match", n, d), ("lit", rng.randrange(33, 127))]
        out.append((name, [toks], {}))
    # full alphabets with few symbols used; the lone distance code; no distance code; 15 bits with 15 bits
    few = lits(b"ACGTACGGT\n") + [("match", 5, 4), ("match", 20, 3), ("lit", 10)]
    out.append(("full alphabets", [few], {"full": True, "trim": False}))
    out.append(("lone distance code", [lits(b"GATTACA") + [("match", 30, 7), ("lit", 10), ("match", 200, 7)]], {"lone": True}))
    out.append(("lone distance code, untrimmed", [lits(b"GATTACA") + [("match", 30, 5), ("lit", 10), ("match", 6, 6)]], {"lone": True, "trim": False}))
    out.append(("no distance code", [_filler(rng, 500)], {}))
    out.append(("no distance code, untrimmed", [_filler(rng, 50)], {"trim": False}))
    both = _filler(rng, 400)
    for d in (1, 3, 24, 100, 390):
        both += [("match", rng.choice((3, 11, 40, 258)), d), ("lit", 10)]
    out.append(("15 bits with 15 bits", [both], {"full": True}))
    out.append(("empty block", [[]], {}))
    out.append(("literal then nothing", [lits(b"A"), [], []], {}))
    return out


def _block_mix(seed, n_blocks=120):
    """120 blocks of every kind in random order in one stream, ending in an empty stored block"""
    rng = random.Random(seed)
    st = Stream("block mix %d" % seed)
    kinds = ["stored0", "stored1", "fixed0", "dynamic0", "fdf", "stored", "fixed", "dynamic"]
    order = [kinds[i % len(kinds)] for i in range(n_blocks - 1)]
    rng.shuffle(order)

    def some():
        t = _filler(rng, rng.randint(1, 30))
        if len(st.text) + len(t) > 8 and rng.random() < 0.7:
            t.append(("match", rng.choice((3, 9, 70, 258)), rng.randint(1, len(st.text) + len(t))))
        return t

    def dyn(toks):
        ll, dl = make_codes(toks, rng, rng.choice(("deepest", "random")), trim=rng.random() < 0.5)
        st.dynamic(toks, ll, dl, rle=rng.random() < 0.5, hclen19=rng.random() < 0.5, deep_clc=rng.random() < 0.5, rng=rng)
    for kind in order:
        if kind == "stored0":
            st.stored(b"")
        elif kind == "stored1":
            st.stored(bytes([rng.choice(b"ACGT")]))
        elif kind == "stored":
            st.stored(bytes(rng.choice(b"ACGT\n") for _ in range(rng.randint(2, 40))))
        elif kind == "fixed0":
            st.fixed([])
        elif kind == "fixed":
            st.fixed(some())
        elif kind == "dynamic0":
            dyn([])
        elif kind == "dynamic":
            dyn(some())
        else:                                                              # fixed -> dynamic -> fixed (counts as one of the 120)
            st.fixed(some()); dyn(some()); st.fixed(some())
            st.info["blocks"] -= 2
    st.stored(b"", True)
    body, text = st.finish()
    return {"name": st.name, "body": body, "text": text, "info": st.info}


def random_stream(seed, max_text=65536):
    """one random valid stream: random tokens, code shapes, header choices and block mixes; text of at most `max_text` bytes"""
    rng = random.Random(seed)
    st = Stream("random %d" % seed)
    budget = rng.choice((40, 300, 3000, 20000, max_text))
    budget = min(budget, max_text)
    alphabet = rng.choice((b"ACGT", b"ACGTN\n@+FI:,#0123456789", bytes(range(256))))
    n_blocks = rng.choice((1, 1, 2, 5, 30))
    for b in range(n_blocks):
        toks, size = [], len(st.text)
        want = rng.randint(0, max(0, (budget - size) // max(1, n_blocks - b)))
        shadow = 0
        while shadow < want:
            have = size + shadow
            if have and rng.random() < 0.5:
                n = rng.choice((3, 4, 5, 8, 13, 31, 66, 130, 257, 258, rng.randint(3, 258)))
                d = min(have, rng.choice((1, 2, 3, 4, 8, 9, 33, 255, 256, 1024, 4097, 32768, rng.randint(1, 32768))))
                if shadow + n > want + 258 or size + shadow + n > max_text:
                    break
                toks.append(("match", n, d)); shadow += n
            else:
                toks.append(("lit", rng.choice(alphabet))); shadow += 1
        last = b == n_blocks - 1
        kind = rng.choice(("dynamic", "dynamic", "dynamic", "fixed", "stored"))
        if kind == "fixed":
            st.fixed(toks, last)
        elif kind == "stored":
            st.stored(expand(toks, st.text)[len(st.text):], last)
        else:
            ll, dl = make_codes(toks, rng, rng.choice(("deepest", "random", "random", "balanced")), full=rng.random() < 0.2,
                                pad_ll=rng.sample(range(286), rng.randint(0, 60)), pad_d=rng.sample(range(30), rng.randint(0, 12)),
                                trim=rng.random() < 0.6, lone=rng.random() < 0.7, long_used=rng.random() < 0.6)
            st.dynamic(toks, ll, dl, last, rle=rng.random() < 0.8, cross=rng.random() < 0.8, hclen19=rng.random() < 0.3,
                       deep_clc=rng.random() < 0.5, rng=rng)
    body, text = st.finish()
    return {"name": st.name, "body": body, "text": text, "info": st.info}


def valid_corpus(n_random=300, seed=1):
    """every planned valid stream in every encoding that applies, two block mixes, and n_random random streams:
    [{"name", "body", "text", "info"}], each text at most 65,536 bytes (one BGZF member)"""
    rng = random.Random(seed)
    out = []
    for name, blocks, codes in planned_token_lists(seed):
        for how in ENCODINGS:
            if how == "fixed" and codes:
                continue                                                   # (the case is about a dynamic code set)
            out.append(encode(name, blocks, how, rng, **codes))
    # a repeat code that crosses from the literal/length into the distance lengths: 16 over equal lengths, 18 over zeros
    toks = lits(b"ACGT\n") + [("match", 258, 4), ("match", 230, 100)]
    ll = [0] * 286
    for s, l in zip((65, 67, 71, 84, 10, 256, 285, 284), (2, 2, 3, 3, 3, 4, 5, 5)):
        ll[s] = l
    dl = [0] * 30
    for s, l in zip((0, 1, 2, 3, 4, 12, 13), (5, 5, 5, 5, 3, 1, 2)):       # 4/32 + 1/8 + 1/2 + 1/4 = 1
        dl[s] = l
    st = Stream("repeat 16 across HLIT").dynamic(toks, ll, dl, True)
    assert st.info["cross"] == 1
    out.append(dict(zip(("body", "text"), st.finish()), name=st.name, info=st.info))
    ll = [0] * 286
    for s, l in zip((65, 67, 71, 84, 10, 256, 257, 258), (3, 3, 3, 3, 3, 3, 3, 3)):
        ll[s] = l
    dl = [0] * 30
    dl[20], dl[21] = 1, 1
    toks = lits(b"ACGT\n" * 400) + [("match", 3, 1025), ("match", 4, 1537), ("lit", 10)]
    st = Stream("repeat 18 across HLIT").dynamic(toks, ll, dl, True)
    assert st.info["cross"] == 1
    out.append(dict(zip(("body", "text"), st.finish()), name=st.name, info=st.info))
    out += [_block_mix(seed), _block_mix(seed + 1)]
    out += [random_stream(seed * 100000 + i) for i in range(n_random)]
    return out


def corpus_stats(corpus):
    """what the valid streams reach: the longest literal/length and distance code used, streams with a lone distance code, with
    no distance code, with a repeat across HLIT, with a 7-bit code-length code"""
    return {"streams": len(corpus),
            "ll_max": max(c["info"]["ll_max"] for c in corpus), "d_max": max(c["info"]["d_max"] for c in corpus),
            "lone": sum(1 for c in corpus if c["info"]["lone"]), "nodist": sum(1 for c in corpus if c["info"]["nodist"]),
            "cross": sum(1 for c in corpus if c["info"]["cross"]), "clc7": sum(1 for c in corpus if c["info"]["clc_max"] == 7),
            "ll_over_11": sum(1 for c in corpus if c["info"]["ll_max"] > 11), "d_over_8": sum(1 for c in corpus if c["info"]["d_max"] > 8)}


# --- malformed streams --------------------------------------------------------------------------------------------------------
# Each has the defect it is named for and no earlier one.  "zlib": what zlib.decompressobj(-15) says of the raw stream (recorded
# here, checked by the tests); "text": the text a BGZF member around it declares (CRC-32 and ISIZE) — for a stream zlib
# accepts, what it inflates to unless the defect is in that declaration; "level": "deflate" = the raw stream itself is wrong,
# "member" = the stream is fine and the member around it is not; "status": k_bgzf_inflate's reason (hulk::bgzf::status_text).
BAD_SYMBOL = "invalid literal/length or distance symbol"
BAD_CODE = "invalid or over-subscribed Huffman code"
STORED_LEN = "stored block length check failed"
EXHAUSTED = "payload exhausted"
TOO_LONG = "output longer than ISIZE"
TOO_SHORT = "output shorter than ISIZE"
TRAILING = "deflate end not at the payload end"


def malformed_corpus():
    out = []
    head = lits(b"ACGTTGCA\n")
    text = expand(head)

    def add(name, w, zl, status, level="deflate", declared=None):
        body = w if isinstance(w, bytes) else w.getvalue()
        out.append({"name": name, "body": body, "zlib": zl, "status": status, "level": level,
                    "text": text if declared is None else declared})

    def fixed_head():
        w = BitWriter(); w.bits(1, 1); w.bits(1, 2)
        put_tokens(w, head, FIXED_LL, FIXED_D, eob=False)
        return w
    for s in (286, 287):
        w = fixed_head(); w.code(FIXED_LL[s]); w.bits(0, 5); w.code(FIXED_D[0]); w.code(FIXED_LL[EOB])
        add("fixed-code symbol %d" % s, w, "reject", BAD_SYMBOL)
    for s in (30, 31):
        w = fixed_head(); w.code(FIXED_LL[257]); w.code(FIXED_D[s]); w.bits(0, 13); w.code(FIXED_LL[EOB])
        add("fixed-code distance %d" % s, w, "reject", BAD_SYMBOL)
    toks = head + [("match", 4, 3), ("match", 5, 8)]                        # literals, length symbols 258 / 259, distance symbols 2 / 5
    ll_used, d_used = used_symbols(toks)
    good_ll = assign(balanced_lengths(len(ll_used)), sorted(ll_used), 260)
    good_dl = [0, 0, 1, 0, 0, 1]

    def dyn(ll, dl, **kw):
        w = BitWriter()
        dynamic_header(w, ll, dl, True, **kw)
        put_tokens(w, toks, [c or (0, 1) for c in canonical_codes(ll)], [c or (0, 1) for c in canonical_codes(dl)] + [(0, 1)] * 32)
        return w
    assert zlib_verdict(dyn(good_ll, good_dl).getvalue()) == ("accept", expand(toks))      # (the base the defects are put into)
    ll = list(good_ll); ll[259] = 0
    add("incomplete literal/length set", dyn(ll, good_dl), "reject", BAD_CODE)
    add("incomplete distance set (two codes of length 2)", dyn(good_ll, [0, 0, 2, 0, 0, 2]), "reject", BAD_CODE)
    add("lone distance code of length 2", dyn(good_ll, [0, 0, 2]), "reject", BAD_CODE)
    add("over-subscribed distance set", dyn(good_ll, [0, 0, 1, 1, 0, 1]), "reject", BAD_CODE)
    clc = [0] * 19; clc[0] = 1
    add("lone code-length code", dyn(good_ll, good_dl, ops=[(0, 0, 0)] * 266, clc=clc), "reject", BAD_CODE)
    full = assign(balanced_lengths(287), range(287), 287)
    add("HLIT 287", dyn(full, good_dl, hlit=30), "reject", BAD_CODE)
    add("HDIST 31", dyn(good_ll, [5] * 31 + [0], hdist=30, ops=[(v, 0, 0) for v in good_ll + [5] * 31]), "reject", BAD_CODE)
    ll = list(good_ll); ll[EOB] = 0; ll[ord("N")] = good_ll[EOB]                                 # (complete, the code moved to 'N')
    w = BitWriter(); dynamic_header(w, ll, good_dl, True)
    put_tokens(w, head, canonical_codes(ll), canonical_codes(good_dl), eob=False); w.bits(0, 16)
    add("no end-of-block code", w, "reject", BAD_CODE)
    seq = good_ll + good_dl
    add("repeat code 16 first", dyn(good_ll, good_dl, ops=[(16, 2, 0)] + [(v, 0, 0) for v in seq[3:]]), "reject", BAD_CODE)
    add("repeat overruns HLIT + HDIST", dyn(good_ll, good_dl, ops=[(v, 0, 0) for v in seq[:-2]] + [(17, 3, 0)]), "reject", BAD_CODE)
    # the lone 1-bit distance code is 0; a 1 where it is read is the code nobody has
    w = BitWriter(); lone = [0, 0, 1]
    dynamic_header(w, good_ll, lone, True)
    llc = canonical_codes(good_ll)
    put_tokens(w, head, llc, None, eob=False); w.code(llc[258]); w.bits(1, 1); w.code(llc[EOB])
    add("unused bit of a lone 1-bit distance code", w, "reject", BAD_SYMBOL)
    w = BitWriter(); dynamic_header(w, good_ll, [0], True)
    put_tokens(w, head, llc, None, eob=False); w.code(llc[258]); w.bits(0, 1); w.code(llc[EOB])
    add("length symbol when there is no distance code", w, "reject", BAD_SYMBOL)
    w = BitWriter(); w.bits(1, 1); w.bits(0, 2); w.align(); w.raw(struct.pack("<HH", len(text), (len(text) ^ 0xffff) ^ 0x100)); w.raw(text)
    add("stored NLEN mismatch", w, "reject", STORED_LEN)
    w = BitWriter(); w.bits(1, 1); w.bits(0, 2); w.align(); w.raw(struct.pack("<HH", len(text) + 3, (len(text) + 3) ^ 0xffff)); w.raw(text)
    add("stored block longer than the payload", w, "reject", EXHAUSTED, declared=text + b"ACG")
    # the member around a sound stream declares a text one byte shorter / longer, or has a byte behind the final block
    for name, last in (("literal", [("lit", 65)]), ("match", [("match", 3, 2)])):
        st = Stream().fixed(head + last, True)
        body, t = st.finish()
        add("text one byte past ISIZE, by a %s" % name, body, "accept", TOO_LONG, "member", t[:-1])
    st = Stream().fixed(head).stored(b"ACGT", True)
    body, t = st.finish()
    add("text one byte past ISIZE, by a stored block", body, "accept", TOO_LONG, "member", t[:-1])
    body, t = Stream().fixed(head, True).finish()
    add("text short of ISIZE", body, "accept", TOO_SHORT, "member", t + b"A")
    add("a byte of payload behind the final block", body + b"\0", "accept", TRAILING, "member", t)
    return out
