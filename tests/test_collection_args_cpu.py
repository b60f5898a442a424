"""The argument checks of the sketch-collection entry points hulk_cluster, hulk_links, hulk_dendrogram and hulk_linkage: which
message wins when a call breaks two rules at once.

All four open with the same sequence (NULL pointers, n and sketch_size positive, n at most the command's maximum, the metric, the
bottom-k sketch size), then check what is their own (max_distance, band_rows, linkage's method) and close with the flags and the
reserved fields.  Every case below breaks two neighbouring rules of that order and expects the earlier one's text.  The calls go
to the raw ctypes entry points and are refused before the library looks for a device: no GPU needed.
"""
import ctypes

import numpy as np
import pytest

ERR_ARG, ERR_NO_DEVICE = -30, -32
NAN = float("nan")
BAD_METRIC = 2                                                      # (between weightedjaccard and bottomk: no metric)


def _lib():
    from hulk_amd import _lib as lib
    return lib, lib.load()


def call(cmd, *, metric=0, tau=0.5, band=0, method=0, flags=0, reserved=(0, 0, 0, 0), n=3, S=4, mins=True, weights=True,
         outputs=True, opts=True, tiny=False):
    """one call of hulk_<cmd> with these arguments; returns (status, hulk_last_error).  tiny: one-row arrays for an n the call
    refuses before it reads them"""
    lib, L = _lib()
    rows = 1 if tiny else max(n, 1)
    m = np.arange(rows * max(S, 1), dtype=np.uint64); w = np.ones(rows * max(S, 1))
    m_p = m.ctypes.data if mins else None
    w_p = w.ctypes.data if weights else None
    keep = []

    def out(dtype):
        a = np.zeros(rows, dtype=dtype)
        keep.append(a)
        return a.ctypes.data if outputs else None

    count = ctypes.c_uint32(77)
    count_p = ctypes.addressof(count) if outputs else None
    if cmd == "cluster":
        o = lib.ClusterOpts(metric=metric, max_distance=tau, band_rows=band, flags=flags)
    elif cmd == "links":
        o = lib.LinksOpts(metric=metric, max_distance=tau, band_rows=band, flags=flags)
    elif cmd == "dendrogram":
        o = lib.DendrogramOpts(metric=metric, band_rows=band, flags=flags)
    else:
        o = lib.LinkageOpts(metric=metric, method=method, flags=flags)
    for i, v in enumerate(reserved):
        o.reserved[i] = v
    o_p = ctypes.byref(o) if opts else None
    if cmd == "cluster":
        rc = L.hulk_cluster(0, m_p, w_p, n, S, o_p, out(np.uint32), None)
    elif cmd == "links":
        handle = ctypes.c_void_p(0x1234)
        rc = L.hulk_links(0, m_p, w_p, n, S, o_p, ctypes.byref(handle) if outputs else None, None)
        if rc == 0:
            L.hulk_link_list_free(handle)
    elif cmd == "dendrogram":
        rc = L.hulk_dendrogram(0, m_p, w_p, n, S, o_p, out(np.uint32), out(np.uint32), out(np.float64), count_p, None)
    else:
        rc = L.hulk_linkage(0, m_p, w_p, n, S, o_p, out(np.uint32), out(np.uint32), out(np.float64), out(np.uint32), count_p, None)
    return rc, L.hulk_last_error(None).decode()


def max_n(cmd):
    lib, _ = _lib()
    return lib.HULK_LINKAGE_MAX_N if cmd == "linkage" else lib.HULK_CLUSTER_MAX_N


def opening_cases(cmd):
    """the shared opening sequence: NULL, n / sketch_size, n's maximum, metric, bottom-k's sketch size"""
    over = dict(n=max_n(cmd) + 1, S=1, tiny=True)
    return [
        (dict(mins=False, n=0), "NULL"),
        (dict(outputs=False, n=0), "NULL"),
        (dict(opts=False, n=0), "NULL"),
        (dict(weights=False, n=0), "NULL"),                         # (jaccard reads the weights)
        (dict(weights=False, metric=3, n=0), "n and sketch_size must be positive"),      # (bottomk does not)
        (dict(n=0, metric=BAD_METRIC), "n and sketch_size must be positive"),
        (dict(S=0, metric=BAD_METRIC), "n and sketch_size must be positive"),
        (dict(over, metric=BAD_METRIC), f"n must be at most {max_n(cmd)}"),
        (dict(over, metric=3, S=4097), f"n must be at most {max_n(cmd)}"),
    ]


# per command: what it checks between the opening and the closing pair, as (a rule broken, the rule after it broken too, text)
OWN = {
    "cluster": [
        (dict(metric=BAD_METRIC), dict(band=48), "metric"),
        (dict(metric=3, S=4097), dict(tau=NAN), "bottomk takes a sketch_size of at most 4096"),
        (dict(metric=3, S=4097), dict(band=48), "bottomk takes a sketch_size of at most 4096"),
        (dict(tau=-0.25), dict(band=48), "max_distance must be in [0, 1]"),
        (dict(tau=NAN), dict(band=48), "max_distance must be in [0, 1]"),
        (dict(band=48), dict(flags=1), "band_rows must be a multiple of 32"),
    ],
    "links": [
        (dict(metric=BAD_METRIC), dict(band=48), "metric"),
        (dict(metric=3, S=4097), dict(tau=NAN), "bottomk takes a sketch_size of at most 4096"),
        (dict(metric=3, S=4097), dict(band=48), "bottomk takes a sketch_size of at most 4096"),
        (dict(tau=1.5), dict(band=48), "max_distance must be in [0, 1]"),
        (dict(band=48), dict(flags=2), "band_rows must be a multiple of 32"),
    ],
    "dendrogram": [
        (dict(metric=BAD_METRIC), dict(band=48), "metric"),
        (dict(metric=3, S=4097), dict(band=48), "bottomk takes a sketch_size of at most 4096"),
        (dict(band=48), dict(flags=1), "band_rows must be a multiple of 32"),
    ],
    "linkage": [
        (dict(metric=BAD_METRIC), dict(method=3), "metric"),
        (dict(metric=3, S=4097), dict(method=3), "bottomk takes a sketch_size of at most 4096"),
        (dict(method=-1), dict(flags=1), "method"),
    ],
}
# the closing pair: flags the command does not know, then reserved fields
CLOSING_FLAGS = {"cluster": 1, "links": 2, "dendrogram": 1, "linkage": 1}
COMMANDS = tuple(OWN)


@pytest.mark.parametrize("cmd", COMMANDS)
def test_the_earlier_rule_wins(cmd):
    cases = opening_cases(cmd) + [(dict(a, **b), text) for a, b, text in OWN[cmd]]
    cases.append((dict(flags=CLOSING_FLAGS[cmd], reserved=(0, 0, 1, 0)), "unknown flags"))
    for kw, text in cases:
        rc, msg = call(cmd, **kw)
        assert rc == ERR_ARG and msg == f"invalid argument: hulk_{cmd}: {text}", (cmd, kw, rc, msg)
    # each rule of a pair is refused on its own too: the pairs above are pairs of live rules
    for a, b, text in OWN[cmd]:
        for kw in (a, b):
            rc, msg = call(cmd, **kw)
            assert rc == ERR_ARG, (cmd, kw, rc, msg)
    rc, msg = call(cmd, reserved=(0, 0, 1, 0))
    assert rc == ERR_ARG and msg == f"invalid argument: hulk_{cmd}: reserved fields must be zero", (cmd, rc, msg)


@pytest.mark.parametrize("cmd", COMMANDS)
def test_a_valid_call_gets_past_every_check(cmd):
    """here no device is found (HULK_ERR_NO_DEVICE); where there is one the call runs"""
    allowed = {"cluster": 0, "links": 1, "dendrogram": 0, "linkage": 0}[cmd]
    for kw in (dict(), dict(metric=1), dict(metric=3, weights=False, S=4096), dict(n=1), dict(flags=allowed)):
        rc, msg = call(cmd, **kw)
        assert rc in (0, ERR_NO_DEVICE), (cmd, kw, rc, msg)
        if rc == ERR_NO_DEVICE:
            assert msg, (cmd, kw)
