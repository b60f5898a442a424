"""Inputs that take the device FASTQ / FASTA parsers (hulk_fastq.hip) round their scans more than once, and the conditions
that make them do so.  No test lives here: tests/test_parser_inputs_cpu.py holds the generators, the model and the constants
to the source and to the host parser without a GPU, tests/test_gpu_parser_blocks.py runs the cases through the kernels.

The parser is a chain of prefix scans.  Its single-workgroup scans (k_fq_scan_u32, k_fq_scan_maps, k_fq_scan_cnt, k_fa_scan)
walk their input in trips with a carry from trip to trip, and k_fa_class / k_fa_flags / k_fa_emit go round their grid again
when a block holds more lines than the grid has threads.  Whether an input reaches a second or third trip depends on the block
size, the bytes per line and where the reader cuts the file — so every case comes with a `check` that asserts exactly that, on
a restatement of the reader in numpy (the MODEL below), and fails with "the inputs are no test: ..." when it does not.

The model.  The device reader cuts the stream (the file, plus a '\\n' if its last byte is none: ByteSource) at multiples of the
block size.  FASTQ: a block's parse range starts behind the last line that completed a record in the range before it, slot state
0, and ends where the block ends.  FASTA: it starts at the unterminated line the range before it ended in.  A line counts in a
range when its '\\n' lies in it.  The FASTQ slot machine skips an empty line in slots 0 to 2; in none of these inputs does an
empty line meet slot 3 (asserted), so the slot in front of a line is the number of non-empty lines before it, mod 4.
"""
import numpy as np

# ---- what the inputs are sized by: constants and formulas of hulk_fastq.hip / hulk_ingest_device.hip, pinned against the
# source text by test_parser_inputs_cpu.py::test_the_constants_follow_the_sources
FQ_T = 256                      # threads of a workgroup of the index kernels = lines per line workgroup
THREAD_BYTES = 16               # bytes of a thread of k_fq_count / k_fq_lines
FQ_CHUNK = FQ_T * THREAD_BYTES  # bytes per byte workgroup
FQ_TRIP = 8 * FQ_T              # workgroup entries per trip of k_fq_scan_u32 / k_fq_scan_maps / k_fq_scan_cnt
FA_T = FQ_T
FA_TRIP = 16 * FA_T             # chunks of FA_T lines per trip of k_fa_scan
PORCH = 1 << 20                 # bytes in front of a block's own for the tail of the block before
DEFAULT_BLOCK = 16 << 20
MAX_BLOCK = 32 << 20
MAX_TOKEN = 64 * 1024           # a line of this many bytes is bufio.Scanner's error
K, W, S = 11, 5, 32             # every case: reads of w + k - 1 = 15 bases and more
NL, CR = 10, 13

FQ_TRIP_LINES = FQ_TRIP * FQ_T      # 524,288 lines per trip of the FASTQ line scans
FA_TRIP_LINES = FA_TRIP * FA_T      # 1,048,576 lines per trip of k_fa_scan
WIDTHS = (63, 64, 65, 127, 128, 129, 191, 192, 193, 257)       # k_fa_copy: two preloaded halves of 64, then 64 at a time


def fq_line_cap(block):
    return (PORCH + block) // 8 + 1024


def fq_read_cap(block):
    return fq_line_cap(block) // 2


def fa_line_cap(block):
    return (MAX_TOKEN + block) // 2 + 2


def span(length):
    return PORCH + length + 16


def n_chunks(length):
    return (span(length) + FQ_CHUNK - 1) // FQ_CHUNK


def fq_line_wgs(block):
    return (fq_line_cap(block) + FQ_T - 1) // FQ_T


def fa_glw(block, length):
    """workgroups of the grid of k_fa_class / k_fa_flags / k_fa_emit for a block of `length` bytes"""
    nlwg = (fa_line_cap(block) + FA_T - 1) // FA_T
    return min(nlwg, (span(length) // 16 + FA_T - 1) // FA_T + 1)


def effective_block(block_bytes):
    return min(block_bytes or DEFAULT_BLOCK, MAX_BLOCK)


def _need(cond, what):
    assert cond, f"the inputs are no test: {what}"


def _ceil(a, b):
    return -(-a // b)


# ---- the model ------------------------------------------------------------------------------------------------------------
def stream_of(path):
    data = np.fromfile(path, dtype=np.uint8)
    if len(data) and data[-1] != NL:
        data = np.append(data, np.uint8(NL))
    return data


class Lines:
    """the stream's lines as ScanLines cuts them: `end` = offset of the '\\n', `start`, `length` (one trailing CR dropped), `first`"""
    def __init__(self, data):
        self.end = np.flatnonzero(data == NL)
        self.start = np.concatenate(([0], self.end[:-1] + 1)) if len(self.end) else np.zeros(0, np.int64)
        raw = self.end - self.start
        self.raw = raw
        self.length = raw - ((raw > 0) & (data[np.maximum(self.end - 1, 0)] == CR))
        self.first = np.where(self.length > 0, data[np.minimum(self.start, len(data) - 1)], 0) if len(raw) else raw


class Model:
    """Per block b of the stream: rng_start[b] .. blk_end[b] is its parse range in stream bytes, first_line[b] .. end_line[b]
    the range's lines (global line numbers), tail[b] the bytes it leaves to the next block."""
    def __init__(self, path, block, fasta):
        data = stream_of(path)
        self.data, self.block, self.fasta = data, block, fasta
        ln = self.lines = Lines(data)
        n = len(data)
        nb = self.n_blocks = max(_ceil(n, block), 1)
        self.blk_start = np.arange(nb, dtype=np.int64) * block
        self.blk_end = np.minimum(self.blk_start + block, n)
        self.end_line = np.searchsorted(ln.end, self.blk_end, side="left")        # lines whose '\n' lies in front of the block's end
        nonempty = ln.length > 0
        if fasta:
            self.state = None
            nxt_line = self.end_line                                               # behind the last whole line
            nxt_start = np.where(self.end_line > 0, ln.end[np.maximum(self.end_line - 1, 0)] + 1, 0)
        else:
            self.state = (np.cumsum(nonempty) - nonempty) % 4                      # slot in front of every line
            assert not (~nonempty & (self.state == 3)).any(), "an empty line in slot 3: the model does not cover it"
            done = np.flatnonzero(self.state == 3)                                 # the lines that complete a record
            c = np.searchsorted(ln.end[done], self.blk_end, side="left")           # completing lines in front of the block's end
            last = done[np.maximum(c - 1, 0)]
            nxt_line = np.where(c > 0, last + 1, 0)
            nxt_start = np.where(c > 0, ln.end[last] + 1, 0)
            self.n_records = len(done)
        self.first_line = np.concatenate(([0], nxt_line[:-1]))
        self.rng_start = np.concatenate(([0], nxt_start[:-1]))
        self.n_lines = self.end_line - self.first_line
        self.tail = self.blk_end - nxt_start
        self.tail_in = self.blk_start - self.rng_start                             # the tail a block takes over

    def state_before(self, b, j):
        """slot state in front of line j of block b's range"""
        return int(self.state[self.first_line[b] + j])

    def range_lines(self, b):
        return slice(int(self.first_line[b]), int(self.end_line[b]))

    def byte_trips(self, b):
        """trips of k_fq_scan_u32 that hold newlines for block b: the byte workgroups start at the range's start rounded down to
        16 in the raw buffer, where the block's own bytes begin at PORCH"""
        r = self.range_lines(b)
        if r.stop == r.start:
            return 0
        raw0 = PORCH - int(self.tail_in[b])
        a0 = raw0 & ~15
        last = raw0 + int(self.lines.end[r.stop - 1] - self.rng_start[b])
        return (last - a0) // FQ_CHUNK // FQ_TRIP + 1

    def line_trips(self, b):
        """trips of k_fq_scan_maps / k_fq_scan_cnt that hold lines"""
        return _ceil(_ceil(int(self.n_lines[b]), FQ_T), FQ_TRIP)

    def fa_scan_trips(self, b):
        return _ceil(_ceil(int(self.n_lines[b]), FA_T), FA_TRIP)

    def fa_grid_rounds(self, b):
        glw = fa_glw(self.block, int(self.blk_end[b] - self.blk_start[b]))
        return _ceil(_ceil(int(self.n_lines[b]), FA_T), glw)

    def takeover(self):
        """(block, reasons) of the first FASTQ block the device parser hands to the host, or None: a tail longer than the porch,
        more lines or reads than the index holds, a line of 64 KiB, a header without '@'"""
        ln = self.lines
        for b in range(self.n_blocks):
            if self.tail_in[b] > PORCH:
                return b, ["tail"]
            r = self.range_lines(b)
            why = []
            if self.n_lines[b] > fq_line_cap(self.block):
                why.append("lines")
            seq = (self.state[r] == 1) & (ln.length[r] > 0)
            if seq.sum() > fq_read_cap(self.block) or ln.length[r][seq].sum() > PORCH + self.block:
                why.append("reads")
            if (ln.raw[r] >= MAX_TOKEN).any():
                why.append("long")
            if ((self.state[r] == 0) & (ln.length[r] > 0) & (ln.first[r] != ord("@"))).any():
                why.append("badid")
            if why:
                return b, why
        return None

    def report(self):
        """lines per block and the trips each scan takes, for the test's output"""
        out = []
        for b in range(self.n_blocks):
            if self.fasta:
                out.append(f"block {b}: {int(self.n_lines[b])} lines, tail in {int(self.tail_in[b])}; trips: k_fq_scan_u32 {self.byte_trips(b)}, "
                           f"k_fa_scan {self.fa_scan_trips(b)}, grid rounds of k_fa_class/flags/emit {self.fa_grid_rounds(b)}")
            else:
                out.append(f"block {b}: {int(self.n_lines[b])} lines, tail in {int(self.tail_in[b])}; trips: k_fq_scan_u32 {self.byte_trips(b)}, "
                           f"k_fq_scan_maps / k_fq_scan_cnt {self.line_trips(b)}")
        return "\n".join(out)


# ---- the generators -------------------------------------------------------------------------------------------------------
class Case:
    """One input: the file, how to run it, its exact reads and closed-form stats, and the condition that makes it a test."""
    def __init__(self, name, path, fasta, block_bytes, interval, bases, offsets, stats, check, takeover=False):
        self.name, self.path, self.fasta, self.block_bytes, self.interval = name, path, fasta, block_bytes, interval
        self.bases, self.offsets, self.stats = bases, offsets, stats          # stats: (n_seqs, total_len, n_lines)
        self._check, self.takeover = check, takeover                          # takeover: the host parser must (not) take the FASTQ stream over
        self._model = None

    @property
    def block(self):
        return effective_block(self.block_bytes)

    def model(self):
        if self._model is None:
            self._model = Model(self.path, self.block, self.fasta)
        return self._model

    def check(self):
        m = self.model()
        _need(int(self.offsets[-1]) == len(self.bases) == self.stats[1] and len(self.offsets) - 1 == self.stats[0], "reads and stats disagree")
        _need(len(m.lines.end) == self.stats[2], f"{len(m.lines.end)} lines in the file, {self.stats[2]} in the closed form")
        if not self.fasta:
            _need(m.n_records == self.stats[0], f"{m.n_records} records complete in the model, {self.stats[0]} in the closed form")
        self._check(self, m)
        return m


def _reads(first, n, L):
    from hulk_amd import synth
    bases, offsets = synth.reads_numpy(first, n, L)
    return bases, offsets


def _fastq_rows(bases, n, L):
    """n records `@r\\n` + L bases + `\\n+\\n` + L quality bytes + `\\n` as rows of 2 L + 7 bytes"""
    rows = np.full((n, 2 * L + 7), ord("I"), dtype=np.uint8)
    rows[:, 0] = ord("@"); rows[:, 1] = ord("r"); rows[:, 2] = NL
    rows[:, 3:3 + L] = bases.reshape(n, L)
    rows[:, 3 + L] = NL; rows[:, 4 + L] = ord("+"); rows[:, 5 + L] = NL; rows[:, 6 + 2 * L] = NL
    return rows


def _with_extras(rows, nl_cols, crlf, empties):
    """the rows' bytes with a CR in front of every '\\n' (columns nl_cols) of the records in `crlf`, and empties[r] empty lines in
    front of record r (CR/LF ones in front of a CR/LF record): one np.insert"""
    n, width = rows.shape
    cr_rec = np.flatnonzero(crlf)
    pos = [(cr_rec[:, None] * width + np.asarray(nl_cols)[None, :]).ravel()]
    val = [np.full(len(pos[0]), CR, dtype=np.uint8)]
    for r in np.flatnonzero(empties):
        e = int(empties[r])
        v = [CR, NL] * e if crlf[r] else [NL] * e
        pos.append(np.full(len(v), r * width, dtype=np.int64)); val.append(np.asarray(v, dtype=np.uint8))
    pos, val = np.concatenate(pos), np.concatenate(val)
    order = np.argsort(pos, kind="stable")
    return np.insert(rows.ravel(), pos[order], val[order])


def fastq_short_records(path, n, seed=0, L=15, interval=4000, block_bytes=0, check=None):
    """case 1: n four-line records of 37 bytes, 1 to 3 empty lines in front of about one header in a thousand, CR/LF on every
    seventh record"""
    rng = np.random.default_rng(seed)
    bases, offsets = _reads(0, n, L)
    crlf = np.arange(n) % 7 == 3
    empties = np.where(rng.random(n) < 1e-3, rng.integers(1, 4, n), 0)
    _with_extras(_fastq_rows(bases, n, L), (2, 3 + L, 5 + L, 6 + 2 * L), crlf, empties).tofile(path)
    return Case("fastq line scans", path, False, block_bytes, interval, bases, offsets, (n, n * L, 4 * n + int(empties.sum())),
                check or check_line_scans)


def fastq_clean_records(path, n, L=150, interval=4000, block_bytes=24 << 20, check=None):
    """case 2: n clean records of 2 L + 7 bytes, the last line unterminated"""
    bases, offsets = _reads(0, n, L)
    _fastq_rows(bases, n, L).ravel()[:-1].tofile(path)
    return Case("fastq byte scan", path, False, block_bytes, interval, bases, offsets, (n, n * L, 4 * n), check or check_byte_scan)


def fasta_short_lines(path, n, crlf_every=0, interval=4000, block_bytes=0, check=None):
    """case 3: n records `>r\\n` + five lines of 4 bases (28 bytes, six lines); crlf_every = c: CR/LF on every c-th record"""
    L, per, nper = 20, 4, 5
    bases, offsets = _reads(0, n, L)
    rows = np.full((n, 3 + nper * (per + 1)), NL, dtype=np.uint8)
    rows[:, 0] = ord(">"); rows[:, 1] = ord("r")
    b2 = bases.reshape(n, L)
    for j in range(nper):
        rows[:, 3 + j * (per + 1):3 + j * (per + 1) + per] = b2[:, j * per:(j + 1) * per]
    if crlf_every:
        nl_cols = [2] + [3 + j * (per + 1) + per for j in range(nper)]
        data = _with_extras(rows, nl_cols, np.arange(n) % crlf_every == 1, np.zeros(n, dtype=np.int64))
    else:
        data = rows.ravel()
    data.tofile(path)
    return Case("fasta trips" + (" cr/lf" if crlf_every else ""), path, True, block_bytes, interval, bases, offsets, (n, n * L, n * (1 + nper)),
                check or check_fasta_trips)


def fastq_porch_edge(path, over, block_bytes=8 << 20, L=150, n_after=3000, interval=5000):
    """case 4: clean records up to block - PORCH (- 1 with `over`: one early header is a byte shorter), then a record whose header is
    followed by PORCH empty lines — it completes in block 1 and the tail of block 0 is PORCH (+ 1) bytes"""
    block = effective_block(block_bytes)
    rec = 2 * L + 7
    n0 = (block - PORCH) // rec
    pad = block - PORCH - n0 * rec
    if pad == 0:                                            # (there has to be a header to shorten)
        n0 -= 1; pad = rec
    n = n0 + 1 + n_after
    bases, offsets = _reads(0, n, L)
    rows = _fastq_rows(bases, n, L)
    gap = rows[n0].tobytes()
    early = 100
    with open(path, "wb") as fh:
        fh.write(rows[:early].tobytes())
        fh.write(b"@r" + b"x" * (pad - (1 if over else 0)) + rows[early].tobytes()[2:])
        fh.write(rows[early + 1:n0].tobytes())
        fh.write(gap[:3] + b"\n" * PORCH + gap[3:])
        fh.write(rows[n0 + 1:].tobytes())
    want = PORCH + (1 if over else 0)

    def check(case, m):
        _need(m.n_blocks == 2 and m.tail[0] == want, f"the tail of block 0 is {int(m.tail[0])} bytes, not {want}")
        _need((m.n_lines <= fq_line_cap(block)).all(), f"the line index ({fq_line_cap(block)}) does not hold the tail's lines and the block's: {m.n_lines}")
        _need(m.takeover() == ((1, ["tail"]) if over else None), f"the model hands over at {m.takeover()}")

    return Case("fastq porch edge" + (" + 1" if over else ""), path, False, block_bytes, interval, bases, offsets, (n, n * L, 4 * n + PORCH),
                check, takeover=over)


def fastq_line_cap_edge(path, over, block_bytes=131072, interval=4000):
    """case 5: two blocks.  Block 0: a header, then empty lines to its end (no record completes: its tail is the whole block).
    Block 1: empty lines, then the sequence, `+` and the quality line, sized to end the block.  The second range holds exactly
    fq_line_cap lines (+ 1 with `over`: the header is a byte shorter, block 0 an empty line longer)."""
    block = effective_block(block_bytes)
    cap = fq_line_cap(block)
    hdr = b"@r" if over else b"@rr"
    lines0 = 1 + block - (len(hdr) + 1)                     # the header and block 0's empty lines
    e1 = cap + (1 if over else 0) - lines0 - 3              # block 1's empty lines
    two_l = block - e1 - 4
    assert e1 > 0 and two_l % 2 == 0, (e1, two_l)
    L = two_l // 2
    bases, offsets = _reads(0, 1, L)
    with open(path, "wb") as fh:
        fh.write(hdr + b"\n" * (lines0 + e1) + bases.tobytes() + b"\n+\n" + b"I" * L + b"\n")
    want = cap + (1 if over else 0)

    def check(case, m):
        _need(m.n_blocks == 2 and len(m.data) == 2 * block and m.tail[0] == block, f"blocks {m.n_blocks}, bytes {len(m.data)}, tail {int(m.tail[0])}")
        _need(m.n_lines[1] == want, f"the second range holds {int(m.n_lines[1])} lines, not {want}")
        _need(L + 1 < MAX_TOKEN, "a line of 64 KiB")
        _need(m.takeover() == ((1, ["lines"]) if over else None), f"the model hands over at {m.takeover()}")

    return Case("fastq line cap" + (" + 1" if over else ""), path, False, block_bytes, interval, bases, offsets, (1, L, lines0 + e1 + 3),
                check, takeover=over)


def _scatter(path, sizes, groups):
    """records of differing sizes: groups = [(record indices, rows)] -> the file, every record at the sum of the sizes before it"""
    starts = np.cumsum(sizes) - sizes
    out = np.empty(int(sizes.sum()), dtype=np.uint8)
    for idx, rows in groups:
        out[starts[idx][:, None] + np.arange(rows.shape[1])[None, :]] = rows
    out.tofile(path)


def _width_plan(n):
    r = np.arange(n)
    width = np.asarray(WIDTHS)[r % len(WIDTHS)]
    crlf = (r // len(WIDTHS)) % 2 == 1
    return r, width, crlf


def fasta_copy_widths(path, n=3000, per_rec=3, interval=700, block_bytes=131072):
    """case 6, FASTA: record r is `>r` and three lines of WIDTHS[r % 10] bases; every other round of ten with CR/LF"""
    r, width, crlf = _width_plan(n)
    lens = width * per_rec
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.uint64)
    bases = _reads(0, 1, int(lens.sum()))[0]
    eol = 1 + crlf
    sizes = 2 + eol + per_rec * (width + eol)
    groups = []
    for wd in WIDTHS:
        for c in (False, True):
            idx = np.flatnonzero((width == wd) & (crlf == c))
            e = [CR, NL] if c else [NL]
            rows = np.empty((len(idx), int(sizes[idx[0]])), dtype=np.uint8)
            rows[:, 0] = ord(">"); rows[:, 1] = ord("r"); rows[:, 2:2 + len(e)] = e
            at = 2 + len(e)
            src = offsets[idx].astype(np.int64)
            for j in range(per_rec):
                rows[:, at:at + wd] = bases[src[:, None] + j * wd + np.arange(wd)[None, :]]
                rows[:, at + wd:at + wd + len(e)] = e
                at += wd + len(e)
            groups.append((idx, rows))
    _scatter(path, sizes, groups)
    return Case("fasta copy widths", path, True, block_bytes, interval, bases, offsets, (n, int(lens.sum()), n * (1 + per_rec)), check_copy_widths)


def fastq_copy_widths(path, n=3000, interval=700, block_bytes=131072):
    """case 6, FASTQ: read r has WIDTHS[r % 10] bases; every other round of ten with CR/LF"""
    r, width, crlf = _width_plan(n)
    offsets = np.concatenate(([0], np.cumsum(width))).astype(np.uint64)
    bases = _reads(0, 1, int(width.sum()))[0]
    eol = 1 + crlf
    sizes = 2 + 2 * width + 1 + 4 * eol
    groups = []
    for wd in WIDTHS:
        for c in (False, True):
            idx = np.flatnonzero((width == wd) & (crlf == c))
            e = [CR, NL] if c else [NL]
            k = len(e)
            rows = np.full((len(idx), int(sizes[idx[0]])), ord("I"), dtype=np.uint8)
            rows[:, 0] = ord("@"); rows[:, 1] = ord("r"); rows[:, 2:2 + k] = e
            at = 2 + k
            rows[:, at:at + wd] = bases[offsets[idx].astype(np.int64)[:, None] + np.arange(wd)[None, :]]
            rows[:, at + wd:at + wd + k] = e
            rows[:, at + wd + k] = ord("+"); rows[:, at + wd + k + 1:at + wd + 2 * k + 1] = e
            rows[:, -k:] = e
            groups.append((idx, rows))
    _scatter(path, sizes, groups)
    return Case("fastq copy widths", path, False, block_bytes, interval, bases, offsets, (n, int(width.sum()), 4 * n), check_copy_widths)


# ---- the conditions -------------------------------------------------------------------------------------------------------
def check_line_scans(case, m):
    """some block's line scans carry a slot state other than 0 into their second and their third trip, and the two differ"""
    _need(case.block_bytes == 0 and m.block == DEFAULT_BLOCK, "not the default block")
    _need(m.n_blocks >= 3, f"{m.n_blocks} blocks: blocks 1 and 2 have a tail")
    _need(m.takeover() is None, f"the device parser hands over at {m.takeover()}")
    _need((m.n_lines <= fq_line_cap(m.block)).all(), "a range outgrows the line index")
    _need(_ceil(fq_line_wgs(m.block), FQ_TRIP) >= 3, "the line scans end before their third trip")
    good = []
    for b in range(m.n_blocks):
        if m.n_lines[b] <= 2 * FQ_TRIP_LINES + FQ_T:
            continue
        s1, s2 = m.state_before(b, FQ_TRIP_LINES), m.state_before(b, 2 * FQ_TRIP_LINES)
        if s1 != 0 and s2 != 0 and s1 != s2:
            good.append(b)
    _need(good, "no block whose slot states in front of lines %d and %d are non-zero and differ" % (FQ_TRIP_LINES, 2 * FQ_TRIP_LINES))
    _need(any(m.line_trips(b) >= 3 and m.tail_in[b] > 0 and m.byte_trips(b) >= 3 for b in range(1, m.n_blocks)),
          "no block with a tail whose byte scan reaches its third trip")
    ln = m.lines
    _need((ln.length == 0).sum() >= 100 and (ln.raw != ln.length).sum() >= 1000, "hardly any empty or CR/LF lines")
    return good


def check_byte_scan(case, m):
    """the first block has no tail and its chunks fill three whole trips of k_fq_scan_u32, all of them with newlines"""
    _need(m.block // FQ_CHUNK == 3 * FQ_TRIP and m.block % FQ_CHUNK == 0, f"{m.block / FQ_CHUNK} chunks are not three whole trips")
    _need(m.n_blocks == 2 and m.blk_end[0] == m.block, "not a little over one block")
    _need(m.takeover() is None, f"the device parser hands over at {m.takeover()}")
    _need(np.fromfile(case.path, dtype=np.uint8)[-1] != NL, "the last line is terminated")
    end = m.lines.end[m.range_lines(0)]
    per_trip = np.bincount(end // FQ_CHUNK // FQ_TRIP, minlength=3)
    _need(len(per_trip) == 3 and (per_trip > 0).all(), f"newlines per trip of block 0: {per_trip}")
    _need((end // FQ_CHUNK >= 2 * FQ_TRIP).sum() > FQ_TRIP, "chunks 4096 and up of the first range hold hardly any newlines")
    _need(m.byte_trips(0) == 3, f"the model counts {m.byte_trips(0)} trips")
    return per_trip


def check_fasta_trips(case, m):
    """some block's k_fa_scan takes a third trip and its grids go round a fourth time, headers and sequence lines in every one"""
    _need(case.block_bytes == 0 and m.block == DEFAULT_BLOCK, "not the default block")
    ln = m.lines
    _need((ln.length > 0).all(), "an empty line ends the parsing")
    _need((m.n_lines <= fa_line_cap(m.block)).all(), "a range outgrows the line index")
    good = []
    for b in range(m.n_blocks):
        live = int(m.n_lines[b])
        per_round = fa_glw(m.block, int(m.blk_end[b] - m.blk_start[b])) * FA_T
        if live <= 2 * FA_TRIP_LINES + FA_T or live <= 3 * per_round:
            continue
        hdr = ln.first[m.range_lines(b)] == ord(">")
        both = True
        for step in (FA_TRIP_LINES, per_round):
            for at in range(0, live, step):
                part = hdr[at:at + step]
                both = both and part.any() and not part.all()
        if both:
            good.append(b)
    _need(good, "no block with more than 2 x %d + %d lines and more than three rounds of its grid" % (FA_TRIP_LINES, FA_T))
    _need(m.n_blocks >= 2, "one block only")
    return good


def check_copy_widths(case, m):
    """every width is there as a sequence line with '\\n' and with CR/LF, in more than one block"""
    ln = m.lines
    _need(m.n_blocks >= 3, f"{m.n_blocks} blocks")
    if not case.fasta:
        _need(m.takeover() is None, f"the device parser hands over at {m.takeover()}")
    seq = ln.first != ord(">") if case.fasta else (m.state == 1)
    for wd in WIDTHS:
        for cr in (0, 1):
            _need(((ln.length == wd) & (ln.raw - ln.length == cr) & seq).sum() >= 10, f"width {wd}, cr {cr}")
    _need(sorted(set(np.diff(case.offsets.astype(np.int64)).tolist())) == sorted(set(w * (3 if case.fasta else 1) for w in WIDTHS)), "read lengths")


# ---- the cases ------------------------------------------------------------------------------------------------------------
LINE_SCANS_SEED = 3             # (its empty lines leave blocks 0 and 1 the slot states check_line_scans asks for: 3 2 1 and 3 2 2
                                #  in front of their second, third and fourth trip; about three seeds in eight leave none)
CASES = ("fastq_line_scans", "fastq_byte_scan", "fasta_trips", "fasta_trips_crlf", "fastq_porch_edge", "fastq_porch_edge_over",
         "fastq_line_cap", "fastq_line_cap_over", "fasta_copy_widths", "fastq_copy_widths")
SCALED = ("fastq_line_scans", "fasta_trips", "fasta_trips_crlf")       # also written at 1/50 of their size for oracle/linepump.py


def build(name, tmp, scale=1):
    """the case `name`, its file written into directory `tmp`; scale = 50: the same generator at 1/50 of the records (no check)"""
    import os
    p = os.path.join(str(tmp), name + (".fa" if name.startswith("fasta") else ".fq"))
    none = (lambda case, m: None) if scale != 1 else None
    if name == "fastq_line_scans":          # a little more than two default blocks of 37-byte records: about 40 MB
        return fastq_short_records(p, (2 * DEFAULT_BLOCK + 6_500_000) // 37 // scale, seed=LINE_SCANS_SEED, check=none)
    if name == "fastq_byte_scan":           # a little over one block of 24 MiB
        return fastq_clean_records(p, ((24 << 20) + 600_000) // 307)
    if name == "fasta_trips":               # a little over one default block of 28-byte records
        return fasta_short_lines(p, (DEFAULT_BLOCK + 600_000) // 28 // scale, check=none)
    if name == "fasta_trips_crlf":          # CR/LF on every fourth record: 29.5 bytes a record keep the lines above three grid rounds
        return fasta_short_lines(p, (DEFAULT_BLOCK + 600_000) // 28 // scale, crlf_every=4, check=none)
    if name == "fastq_porch_edge":
        return fastq_porch_edge(p, False)
    if name == "fastq_porch_edge_over":
        return fastq_porch_edge(p, True)
    if name == "fastq_line_cap":
        return fastq_line_cap_edge(p, False)
    if name == "fastq_line_cap_over":
        return fastq_line_cap_edge(p, True)
    if name == "fasta_copy_widths":
        return fasta_copy_widths(p)
    if name == "fastq_copy_widths":
        return fastq_copy_widths(p)
    raise KeyError(name)
