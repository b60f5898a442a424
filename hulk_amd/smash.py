"""`hulk smash` on the GPU: pairwise similarity matrix of a directory of HULK sketches.

Reference: cmd/smash.go:60-226 (parameter checks, CollectJSONs, makeMatrix), HULKdata.GetDistance
(src/sketchio/sketchio.go:259-306), distances.GetDistance/GetWJD (src/distances/distances.go).
The N x N x S comparison runs in libhulkhip (hulk_smash); this module only loads, orders and writes.
search / search_files: for every query sketch the k closest sketches of a database (hulk_search, hulk_search_files) — the same
distance, selected on the GPU while the database streams through it.
cluster / cluster_files: the connected components of "distance <= threshold" over a collection (hulk_cluster, hulk_cluster_files):
single linkage, without the N x N matrix.
dendrogram / dendrogram_files: every threshold at once — the minimum spanning forest of the distance graph (hulk_dendrogram,
hulk_dendrogram_files); cut_dendrogram and linkage_matrix read it on the host.
linkage / linkage_files: the single-, complete- or average-linkage dendrogram by agglomeration over the N x N matrix, which stays on the
device (hulk_linkage, hulk_linkage_files); cut_dendrogram and linkage_matrix read its merges too.
"""
import ctypes
import fnmatch
import glob
import os

import numpy as np

from . import _lib
from ._lib import HulkError
from .sketchio import load_hulk_data

# cmd/smash.go:30 (the others are unreachable from the CLI), and "bottomk": the set similarity of two KMV sketches
# (KMVsketch.GetSimilarity, kmv.go:119-159, which the reference never reaches from its command line) — kmv sketches only
AVAIL_METRICS = ["jaccard", "weightedjaccard", "bottomk"]
PANEL_METRICS = ["jaccard", "weightedjaccard"]          # panels score histosketch snapshots
_METRIC_CODE = {"jaccard": _lib.HULK_METRIC_JACCARD, "weightedjaccard": _lib.HULK_METRIC_WEIGHTED_JACCARD, "bottomk": _lib.HULK_METRIC_BOTTOMK}
AVAIL_ALGORITHMS = ["histosketch", "kmv", "khf"]        # sketchio.go:17
AVAIL_LINKAGES = ["single", "complete", "average"]
_LINKAGE_CODE = {"single": _lib.HULK_LINKAGE_SINGLE, "complete": _lib.HULK_LINKAGE_COMPLETE, "average": _lib.HULK_LINKAGE_AVERAGE}


def _check_metric(metric, avail=AVAIL_METRICS):
    if metric not in avail:
        raise HulkError(-30, f"supplied distance metric is not available: {metric}\nplease select one of the following: {avail}")


def _check_algo(algo):
    if algo not in AVAIL_ALGORITHMS:
        raise HulkError(-30, f"supplied algorithm not available: {algo}\nplease select one of the following: {AVAIL_ALGORITHMS}")


def _check_linkage(method):
    if method not in AVAIL_LINKAGES:
        raise HulkError(-30, f"supplied linkage is not available: {method}\nplease select one of the following: {AVAIL_LINKAGES}")


def _sketch_arrays(mins, weights, metric):
    """(mins as contiguous uint64, weights as _weights_for gives them), both [n][sketch_size]"""
    m = np.ascontiguousarray(mins, dtype=np.uint64)
    w = _weights_for(metric, m, weights)
    if m.ndim != 2 or (w is not None and m.shape != w.shape):
        raise ValueError("mins/weights must be [n][sketch_size]")
    return m, w


def _band_rows(band_rows):
    band_rows = int(band_rows)
    if not 0 <= band_rows < 2 ** 32:
        raise ValueError("band_rows must be a multiple of 32 (0 = default)")
    return band_rows


def _u32_or_zero(x):
    """x as a uint32 argument; out of range: 0, which the library refuses"""
    return x if 0 <= x < 2 ** 32 else 0


def _fs(path):
    return None if path is None else os.fsencode(path)


def _ptr(a):
    return None if a is None else a.ctypes.data


def _call(fn, *args):
    """a direct call into the library: HulkError with hulk_last_error's text when it fails"""
    rc = fn(*args)
    if rc != 0:
        raise HulkError(rc, _lib.load().hulk_last_error(None).decode("utf-8", "replace"))


def _call_files(fn, *args):
    """a *_files call: the library writes its text into the 4096-byte error buffer appended to args"""
    err = ctypes.create_string_buffer(4096)
    rc = fn(*args, err, len(err))
    if rc != 0:
        raise HulkError(rc, err.value.decode("utf-8", "replace"))


def _stats(st):
    """a stats struct as a dict, one key per field"""
    return {name: getattr(st, name) for name, _ in st._fields_}


def _make_parent_dir(path):
    """the directory of an output file, created (0700) when it does not exist"""
    od = os.path.dirname(path)
    if od and od != "." and not os.path.exists(od):
        os.makedirs(od, mode=0o700)


def collect_jsons(sketch_dir, recursive=False):
    """helpers.CollectJSONs (src/helpers/helpers.go:168-208)."""
    if not sketch_dir.endswith("/"):
        sketch_dir += "/"
    if recursive:
        found = []
        for root, _, files in os.walk(sketch_dir):
            found += [os.path.join(root, f) for f in sorted(files) if fnmatch.fnmatch(f, "*.json")]
    else:
        found = glob.glob(sketch_dir + "*.json")
    if not found:
        raise HulkError(-30, f"no JSON files found in supplied directory: {sketch_dir}\n")
    return found


def distance_matrix(mins, weights, metric="jaccard", device=0, timing=None):
    """distances[s, q] = GetDistance(subject s, query q) for all pairs, computed on the GPU.
    timing: a dict that receives "kernel_ms" (k_smash alone, HIP events; hulk_smash_ex).
    metric "bottomk": 1 - (multiset intersection of the two rows of mins, as uint64) / sketch_size, whatever the order of a row's
    values; weights is not read and may be None."""
    mins = np.ascontiguousarray(mins, dtype=np.uint64)
    weights = _weights_for(metric, mins, weights)
    if (weights is not None and mins.shape != weights.shape) or mins.ndim != 2:
        raise ValueError("mins/weights must be [n_sketches][sketch_size]")
    n, s = mins.shape
    out = np.zeros((n, n), dtype=np.float64)
    kms = ctypes.c_double(0.0)
    try:
        _call(_lib.load().hulk_smash_ex, device, mins.ctypes.data, _ptr(weights), n, s, _METRIC_CODE.get(metric, _lib.HULK_METRIC_JACCARD),
              out.ctypes.data, ctypes.byref(kms) if timing is not None else None)
    finally:
        if timing is not None:
            timing["kernel_ms"] = kms.value
    return out


def _weights_for(metric, mins, weights):
    """weights as a contiguous float64 array; None stays None for bottomk, which reads none"""
    if weights is None and metric == "bottomk":
        return None
    return np.ascontiguousarray(weights, dtype=np.float64)


def panel_distances(snap_mins, snap_weights, panel_mins, panel_weights, metric="jaccard", role="row", device=0):
    """distances[i, p] between sketch i of snap_* [m][S] and sketch p of panel_* [n_panel][S], on the GPU with the kernel that
    scores sketch snapshots against a panel (hulk_panel_distances): role "row" = sketch i is the subject (the block
    distance_matrix([snap; panel])[:m, m:]), "column" = panel sketch p is (the block [m:, :m] transposed).  One against many."""
    _check_metric(metric, PANEL_METRICS)
    if role not in ("row", "column"):
        raise ValueError("role must be 'row' or 'column'")
    sm = np.ascontiguousarray(snap_mins, dtype=np.uint64); sw = np.ascontiguousarray(snap_weights, dtype=np.float64)
    pm = np.ascontiguousarray(panel_mins, dtype=np.uint64); pw = np.ascontiguousarray(panel_weights, dtype=np.float64)
    if sm.ndim != 2 or pm.ndim != 2 or sm.shape != sw.shape or pm.shape != pw.shape:
        raise ValueError("mins/weights must be [n][sketch_size]")
    if sm.shape[1] != pm.shape[1]:
        raise HulkError(-30, f"sketch length mismatch: {sm.shape[1]} vs {pm.shape[1]}\n")
    out = np.zeros((sm.shape[0], pm.shape[0]), dtype=np.float64)
    _call(_lib.load().hulk_panel_distances, device, sm.ctypes.data, sw.ctypes.data, sm.shape[0], pm.ctypes.data, pw.ctypes.data, pm.shape[0],
          sm.shape[1], _METRIC_CODE[metric], _lib.HULK_PANEL_COLUMN if role == "column" else _lib.HULK_PANEL_ROW, out.ctypes.data)
    return out


def _search_consts(metric, role):
    _check_metric(metric)
    if role not in ("row", "column"):
        raise ValueError("role must be 'row' or 'column'")
    return (_METRIC_CODE[metric],
            _lib.HULK_PANEL_COLUMN if role == "column" else _lib.HULK_PANEL_ROW)


def search(q_mins, q_weights, db_mins, db_weights, k, metric="jaccard", role="row", max_distance=None, self_search=False,
           scratch_bytes=0, device=0, stats=None):
    """For every query sketch the k closest sketches of a database, on the GPU (hulk_search): -> (index[m][k] uint32,
    distance[m][k], count[m]).  The distance is distance_matrix's for that pair — role "row": the query is the subject, "column":
    the database sketch is — and a query's hits are the pairs whose distance is not NaN (and <= max_distance, if given in [0, 1]),
    ordered by (distance, database index), cut to k; behind count[i] the entries are 0xFFFFFFFF / NaN.  self_search: db_mins and
    db_weights are None, the queries are searched among themselves and the pair (i, i) is left out.  The database streams through
    the device in strips sized by scratch_bytes (0 = 1 GiB): no m x n_db array exists.  stats: a dict that receives
    seconds_total, kernel_ms_dist, kernel_ms_select, strips, query_blocks."""
    metric_c, role_c = _search_consts(metric, role)
    qm, qw = _sketch_arrays(q_mins, q_weights, metric)
    if self_search:
        if db_mins is not None or db_weights is not None:
            raise ValueError("self_search takes no database")
        dm = dw = None
    else:
        dm, dw = _sketch_arrays(db_mins, db_weights, metric)
        if qm.shape[1] != dm.shape[1]:
            raise HulkError(-30, f"sketch length mismatch: {qm.shape[1]} vs {dm.shape[1]}\n")
    m, k = qm.shape[0], int(k)
    o = _lib.SearchOpts(k=_u32_or_zero(k), metric=metric_c, role=role_c, flags=_lib.HULK_SEARCH_SELF if self_search else 0,
                        max_distance=-1.0 if max_distance is None else float(max_distance), scratch_bytes=int(scratch_bytes))
    kk = max(min(k, _lib.HULK_SEARCH_MAX_K), 1)
    index = np.zeros((m, kk), dtype=np.uint32); dist = np.zeros((m, kk), dtype=np.float64); count = np.zeros(m, dtype=np.uint32)
    st = _lib.SearchStats()
    _call(_lib.load().hulk_search, device, qm.ctypes.data, _ptr(qw), m, _ptr(dm), _ptr(dw), 0 if dm is None else dm.shape[0], qm.shape[1],
          ctypes.byref(o), index.ctypes.data, dist.ctypes.data, count.ctypes.data, ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return index, dist, count


def search_files(query_files, db_files, k, ksize=21, algo="histosketch", metric="jaccard", role="row", max_distance=None,
                 self_search=False, csv_path=None, threads=0, device=0, stats=None):
    """The directory form (hulk_search_files): both lists of sketch files are loaded and MD5-verified by the native loader (a single
    query file is fine), the search runs on the GPU and, csv_path given, the library writes "query,rank,hit,similarity" — one line
    per hit, the similarity the string `smash` prints for that pair.  -> (query ordering, database ordering, index, distance, count);
    the orderings are the sorted unique paths, index counts the database's."""
    _search_consts(metric, role)
    _check_algo(algo)
    q_order = sorted(set(query_files))
    d_order = q_order if self_search else sorted(set(db_files))
    k = int(k)
    kk = max(min(k, _lib.HULK_SEARCH_MAX_K), 1)
    m = len(q_order)
    index = np.zeros((m, kk), dtype=np.uint32); dist = np.zeros((m, kk), dtype=np.float64); count = np.zeros(max(m, 1), dtype=np.uint32)
    qa, nq = _paths(query_files)
    da, nd = (None, 0) if self_search else _paths(db_files)
    st = _lib.SearchStats()
    _call_files(_lib.load().hulk_search_files, device, qa, nq, da, nd, ksize, algo.encode(), metric.encode(), 1 if role == "column" else 0,
                _u32_or_zero(k), -1.0 if max_distance is None else float(max_distance), _lib.HULK_SEARCH_SELF if self_search else 0, threads,
                _fs(csv_path), index.ctypes.data, dist.ctypes.data, count.ctypes.data, ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return q_order, d_order, index, dist, count[:m]


class Index:
    """A banded index over a sketch collection that stays on the GPU (hulk_index_*): search()'s hit lists under jaccard at a distance
    threshold, computed over the sketches that share a band with the query.  Built for max_distance D with the default bands
    (bands=0: u_max + 1) the result is search(metric="jaccard", the same k and max_distance <= D) over the whole collection, bit for
    bit; with fewer bands it is an LSH filter, faster and incomplete (include/hulk_hip.h states the rule).  One call at a time per
    index; close() (or the end of a `with` block) frees the device memory."""

    def __init__(self, handle):
        self._h = handle

    @staticmethod
    def _opts(max_distance, bands, metric):
        _check_metric(metric)
        bands = int(bands)
        return _lib.IndexOpts(max_distance=float(max_distance), bands=bands if 0 <= bands < 2 ** 32 else 0xFFFFFFFF, metric=_METRIC_CODE[metric])

    @classmethod
    def build(cls, mins, max_distance, bands=0, device=0, names=None, metric="jaccard"):
        """mins [n][S] uint64 -> Index.  names: n strings (search_files' CSV and .names report them)."""
        m = np.ascontiguousarray(mins, dtype=np.uint64)
        if m.ndim != 2:
            raise ValueError("mins must be [n][sketch_size]")
        o = cls._opts(max_distance, bands, metric)
        L = _lib.load()
        h = ctypes.c_void_p()
        _call(L.hulk_index_build, device, m.ctypes.data, m.shape[0], m.shape[1], ctypes.byref(o), ctypes.byref(h))
        ix = cls(h)
        if names is not None:
            try:
                _call(L.hulk_index_set_names, h, *_paths(names))
            except HulkError:
                ix.close()
                raise
        return ix

    @classmethod
    def build_files(cls, files, max_distance, bands=0, ksize=21, algo="histosketch", threads=0, device=0):
        """The sketch files through the native loader (MD5, FindSketch, the reference's error texts); the sorted unique paths are the names."""
        o = cls._opts(max_distance, bands, "jaccard")
        arr, n = _paths(files)
        h = ctypes.c_void_p()
        _call_files(_lib.load().hulk_index_build_files, device, arr, n, ksize, algo.encode(), threads, ctypes.byref(o), ctypes.byref(h))
        return cls(h)

    @classmethod
    def load(cls, path, device=0):
        h = ctypes.c_void_p()
        _call(_lib.load().hulk_index_load, device, os.fsencode(path), ctypes.byref(h))
        return cls(h)

    def _handle(self):
        if self._h is None:
            raise ValueError("the index is closed")
        return self._h

    def save(self, path):
        _call(_lib.load().hulk_index_save, self._handle(), os.fsencode(path))

    @property
    def info(self):
        """dict(n, sketch_size, bands, max_distance, device_bytes)"""
        n, s, b, d, by = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_double(), ctypes.c_uint64()
        _lib.load().hulk_index_info(self._handle(), ctypes.byref(n), ctypes.byref(s), ctypes.byref(b), ctypes.byref(d), ctypes.byref(by))
        return dict(n=n.value, sketch_size=s.value, bands=b.value, max_distance=d.value, device_bytes=by.value)

    @property
    def names(self):
        L = _lib.load()
        return [os.fsdecode(L.hulk_index_name(self._handle(), i)) for i in range(self.info["n"])]

    def _search_opts(self, k, max_distance, self_search, scratch_bytes):
        k = int(k)
        o = _lib.IndexSearchOpts(k=_u32_or_zero(k), flags=_lib.HULK_SEARCH_SELF if self_search else 0,
                                 max_distance=-1.0 if max_distance is None else float(max_distance), scratch_bytes=int(scratch_bytes))
        return o, max(min(k, _lib.HULK_SEARCH_MAX_K), 1)

    def search(self, q_mins, k, max_distance=None, self_search=False, scratch_bytes=0, stats=None):
        """-> (index[m][k] uint32, distance[m][k], count[m]) as search() gives them.  max_distance None: the build's; above the
        build's: HulkError.  self_search: q_mins is None and the queries are the indexed sketches, (i, i) left out.  stats: a dict
        that receives candidates, within, the kernel milliseconds per phase, query_blocks, pieces."""
        h = self._handle()
        if self_search:
            if q_mins is not None:
                raise ValueError("self_search takes no queries")
            qm, m = None, self.info["n"]
        else:
            qm = np.ascontiguousarray(q_mins, dtype=np.uint64)
            if qm.ndim != 2:
                raise ValueError("mins must be [m][sketch_size]")
            if qm.shape[1] != self.info["sketch_size"]:
                raise HulkError(-30, f"sketch length mismatch: {qm.shape[1]} vs {self.info['sketch_size']}\n")
            m = qm.shape[0]
        o, kk = self._search_opts(k, max_distance, self_search, scratch_bytes)
        index = np.zeros((m, kk), dtype=np.uint32); dist = np.zeros((m, kk), dtype=np.float64); count = np.zeros(max(m, 1), dtype=np.uint32)
        st = _lib.IndexSearchStats()
        _call(_lib.load().hulk_index_search, h, _ptr(qm), m, ctypes.byref(o), index.ctypes.data, dist.ctypes.data, count.ctypes.data, ctypes.byref(st))
        if stats is not None:
            stats.update(_stats(st))
        return index, dist, count[:m]

    def search_files(self, query_files, k, max_distance=None, self_search=False, ksize=21, algo="histosketch", csv_path=None, threads=0,
                     stats=None):
        """The query files through the native loader; csv_path: search_files' "query,rank,hit,similarity".
        -> (query ordering, index, distance, count)"""
        h = self._handle()
        q_order = self.names if self_search else sorted(set(query_files))
        m = len(q_order)
        o, kk = self._search_opts(k, max_distance, self_search, 0)
        index = np.zeros((m, kk), dtype=np.uint32); dist = np.zeros((m, kk), dtype=np.float64); count = np.zeros(max(m, 1), dtype=np.uint32)
        qa, nq = (None, 0) if self_search else _paths(query_files)
        st = _lib.IndexSearchStats()
        _call_files(_lib.load().hulk_index_search_files, h, qa, nq, ksize, algo.encode(), threads, ctypes.byref(o), _fs(csv_path),
                    index.ctypes.data, dist.ctypes.data, count.ctypes.data, ctypes.byref(st))
        if stats is not None:
            stats.update(_stats(st))
        return q_order, index, dist, count[:m]

    def close(self):
        if self._h is not None:
            _lib.load().hulk_index_free(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cluster(mins, weights, max_distance, metric="jaccard", band_rows=0, device=0, stats=None):
    """Single-linkage clusters of a sketch collection at a distance threshold, on the GPU (hulk_cluster): -> (labels uint32[N],
    n_clusters).  With D = distance_matrix(mins, weights, metric), sketches i != j are linked when D[i, j] <= max_distance or
    D[j, i] <= max_distance (a NaN never links, equality does); a cluster is a connected component and labels[i] its smallest
    member.  max_distance must be in [0, 1]; band_rows (a multiple of 32, 0 = 2048): the subject rows one kernel launch takes —
    it cannot change the result.  stats: a dict that receives seconds_total, kernel_ms_link, kernel_ms_flatten, links (the
    ordered pairs i != j with D[i, j] <= max_distance), bands, clusters."""
    _check_metric(metric)
    m, w = _sketch_arrays(mins, weights, metric)
    band_rows = _band_rows(band_rows)
    o = _lib.ClusterOpts(metric=_METRIC_CODE[metric], max_distance=float(max_distance), band_rows=band_rows)
    labels = np.zeros(max(m.shape[0], 1), dtype=np.uint32)
    st = _lib.ClusterStats()
    _call(_lib.load().hulk_cluster, device, m.ctypes.data, _ptr(w), m.shape[0], m.shape[1], ctypes.byref(o), labels.ctypes.data, ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return labels[:m.shape[0]], int(st.clusters)


def cluster_files(files, max_distance, ksize=21, algo="histosketch", metric="jaccard", csv_path=None, threads=0, device=0, stats=None):
    """The directory form (hulk_cluster_files): the sketch files are loaded and MD5-verified by the native loader (one file is
    fine), the clustering runs on the GPU and, csv_path given, the library writes "sketch,cluster,size,representative" — one line
    per sketch in sorted path order: the 1-based ordinal of its cluster (ordered by smallest member), the cluster's size and the
    path of its smallest member.  -> (ordering, labels, n_clusters); ordering = the sorted unique paths, labels index it."""
    _check_metric(metric)
    _check_algo(algo)
    ordering = sorted(set(files))
    labels = np.zeros(max(len(ordering), 1), dtype=np.uint32)
    arr, n = _paths(files)
    st = _lib.ClusterStats()
    _call_files(_lib.load().hulk_cluster_files, device, arr, n, ksize, algo.encode(), metric.encode(), float(max_distance), threads, _fs(csv_path),
                labels.ctypes.data, ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return ordering, labels[:len(ordering)], int(st.clusters)


def _take_link_list(L, handle):
    """numpy copies of a hulk_link_list; the list is freed"""
    try:
        n, edges = ctypes.c_uint32(), ctypes.c_uint64()
        L.hulk_link_list_info(handle, ctypes.byref(n), ctypes.byref(edges))

        def copy(ptr, count, dtype):
            if not count:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer(ctypes.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy()
        return (copy(L.hulk_link_list_row_start(handle), n.value + 1, np.uint64), copy(L.hulk_link_list_cols(handle), edges.value, np.uint32),
                copy(L.hulk_link_list_distances(handle), edges.value, np.float64))
    finally:
        L.hulk_link_list_free(handle)


def links(mins, weights, max_distance, metric="jaccard", upper=False, max_edges=0, band_rows=0, device=0, stats=None):
    """The links of a sketch collection as a sparse graph, on the GPU (hulk_links): -> (indptr uint64[N + 1], indices uint32[E],
    distances float64[E]), CSR.  With D = distance_matrix(mins, weights, metric), row i lists every j != i with D[i, j] <=
    max_distance in ascending j (a NaN never is listed, equality is) and distances holds D[i, j] bit for bit; E is cluster()'s
    `links` at the same threshold.  weightedjaccard is directed (the subject's weights on both sides); upper=True keeps j > i only.
    Without upper every metric pays the full square.  max_edges (0 = none): more edges than that is a HulkError that names the cap
    and the count reached (stats["edges"] has the count so far).  band_rows as in cluster(): it cannot change the result.
    scipy.sparse.csr_matrix((distances, indices, indptr), shape=(N, N)) takes the three arrays as they are.  stats: a dict that
    receives seconds_total, kernel_ms_count, kernel_ms_fill, edges, bands, max_degree."""
    _check_metric(metric)
    m, w = _sketch_arrays(mins, weights, metric)
    band_rows, max_edges = _band_rows(band_rows), int(max_edges)
    if not 0 <= max_edges < 2 ** 64:
        raise ValueError("max_edges must be non-negative (0 = no cap)")
    o = _lib.LinksOpts(metric=_METRIC_CODE[metric], max_distance=float(max_distance), band_rows=band_rows,
                       flags=_lib.HULK_LINKS_UPPER if upper else 0, max_edges=max_edges)
    st = _lib.LinksStats()
    handle = ctypes.c_void_p()
    L = _lib.load()
    try:
        _call(L.hulk_links, device, m.ctypes.data, _ptr(w), m.shape[0], m.shape[1], ctypes.byref(o), ctypes.byref(handle), ctypes.byref(st))
    finally:                                                        # (also on failure: the max_edges error leaves the count so far)
        if stats is not None:
            stats.update(_stats(st))
    return _take_link_list(L, handle)


def links_files(files, max_distance, ksize=21, algo="histosketch", metric="jaccard", upper=False, max_edges=0, csv_path=None, threads=0,
                device=0, stats=None):
    """The directory form (hulk_links_files): the sketch files are loaded and MD5-verified by the native loader (one file is fine),
    the links are listed on the GPU and, csv_path given, the library writes "sketch,neighbour,distance,similarity" — one line per
    edge in CSR order: the two paths, the distance as %.17g and the similarity string `smash` prints for the pair.
    -> (ordering, indptr, indices, distances); ordering = the sorted unique paths, which the rows and indices count."""
    _check_metric(metric)
    _check_algo(algo)
    ordering = sorted(set(files))
    arr, n = _paths(files)
    st = _lib.LinksStats()
    handle = ctypes.c_void_p()
    L = _lib.load()
    try:
        _call_files(L.hulk_links_files, device, arr, n, ksize, algo.encode(), metric.encode(), float(max_distance), _lib.HULK_LINKS_UPPER if upper else 0,
                    int(max_edges), threads, _fs(csv_path), ctypes.byref(handle), ctypes.byref(st))
    finally:
        if stats is not None:
            stats.update(_stats(st))
    return (ordering,) + _take_link_list(L, handle)


def dendrogram(mins, weights, metric="jaccard", band_rows=0, device=0, stats=None):
    """The single-linkage dendrogram of a sketch collection, on the GPU (hulk_dendrogram): -> (a uint32[E], b uint32[E], d float64[E]),
    a < b, the edges of the minimum spanning forest in merge order.  With D = distance_matrix(mins, weights, metric) the edge {i, j}
    weighs fmin(D[i, j], D[j, i]) (no edge where both are NaN), edges are ordered by (weight, min(i, j), max(i, j)) and the result
    is what Kruskal gives on that order: E = N - (components of the non-NaN graph), and cut_dendrogram(N, a, b, d, tau) is
    cluster(mins, weights, tau, metric) for every tau.  band_rows (a multiple of 32, 0 = 2048) cannot change the result.  stats: a
    dict that receives seconds_total, kernel_ms_offer, kernel_ms_fold, rounds, bands (per round), edges, components."""
    _check_metric(metric)
    m, w = _sketch_arrays(mins, weights, metric)
    o = _lib.DendrogramOpts(metric=_METRIC_CODE[metric], band_rows=_band_rows(band_rows))
    n = m.shape[0]
    a = np.zeros(max(n, 1), dtype=np.uint32); b = np.zeros(max(n, 1), dtype=np.uint32); d = np.zeros(max(n, 1), dtype=np.float64)
    ne = ctypes.c_uint32(0)
    st = _lib.DendrogramStats()
    _call(_lib.load().hulk_dendrogram, device, m.ctypes.data, _ptr(w), n, m.shape[1], ctypes.byref(o), a.ctypes.data, b.ctypes.data, d.ctypes.data,
          ctypes.byref(ne), ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return a[:ne.value], b[:ne.value], d[:ne.value]


def dendrogram_files(files, ksize=21, algo="histosketch", metric="jaccard", csv_path=None, cut_distance=None, cut_csv_path=None,
                     threads=0, device=0, stats=None):
    """The directory form (hulk_dendrogram_files): the sketch files are loaded and MD5-verified by the native loader (one file is
    fine), the dendrogram is computed on the GPU and, csv_path given, the library writes "merge,sketch_a,sketch_b,distance,
    similarity,size" — one line per merge: its 1-based ordinal, the two paths, the distance as %.17g, the similarity as `smash`
    prints it, the size of the cluster the merge creates.  cut_distance (in [0, 1]) with cut_csv_path: the file cluster_files
    writes at that max_distance, byte for byte.  -> (ordering, a, b, d); ordering = the sorted unique paths, a and b index it."""
    _check_metric(metric)
    _check_algo(algo)
    ordering = sorted(set(files))
    n = max(len(ordering), 1)
    a = np.zeros(n, dtype=np.uint32); b = np.zeros(n, dtype=np.uint32); d = np.zeros(n, dtype=np.float64)
    ne = ctypes.c_uint32(0)
    arr, n_paths = _paths(files)
    st = _lib.DendrogramStats()
    _call_files(_lib.load().hulk_dendrogram_files, device, arr, n_paths, ksize, algo.encode(), metric.encode(), threads, _fs(csv_path),
                float("nan") if cut_distance is None else float(cut_distance), _fs(cut_csv_path),
                a.ctypes.data, b.ctypes.data, d.ctypes.data, ctypes.byref(ne), ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return ordering, a[:ne.value], b[:ne.value], d[:ne.value]


def linkage(mins, weights, method, metric="jaccard", device=0, stats=None):
    """The dendrogram of a sketch collection under "single", "complete" or "average" linkage, on the GPU (hulk_linkage):
    -> (a uint32[M], b uint32[M], d float64[M], size uint32[M]), a < b, the merges in the order performed.  With D =
    distance_matrix(mins, weights, metric) and W = fmin(D, D.T) (+inf where both directions are NaN) the clusters start as the
    singletons, named by their smallest member; the pair (p, q), p < q, smallest under (d(p, q), p, q) merges into p, and d(p, k)
    becomes the min / max / size-weighted mean (each operation rounded on its own) of d(p, k) and d(q, k).  M = N - (components of
    the finite graph).  a and b are members of the merged clusters: cut_dendrogram(N, a, b, d, tau) and linkage_matrix(N, a, b, d)
    read the result as they read dendrogram()'s.  The N x N matrix stays on the device (8 * N * N bytes, N at most 65,536).
    stats: a dict that receives seconds_total, kernel_ms_matrix, kernel_ms_merge, merges, components, rows_rescanned."""
    _check_metric(metric)
    _check_linkage(method)
    m, w = _sketch_arrays(mins, weights, metric)
    o = _lib.LinkageOpts(metric=_METRIC_CODE[metric], method=_LINKAGE_CODE[method])
    n = m.shape[0]
    a = np.zeros(max(n, 1), dtype=np.uint32); b = np.zeros(max(n, 1), dtype=np.uint32); d = np.zeros(max(n, 1), dtype=np.float64)
    size = np.zeros(max(n, 1), dtype=np.uint32)
    nm = ctypes.c_uint32(0)
    st = _lib.LinkageStats()
    _call(_lib.load().hulk_linkage, device, m.ctypes.data, _ptr(w), n, m.shape[1], ctypes.byref(o), a.ctypes.data, b.ctypes.data,
          d.ctypes.data, size.ctypes.data, ctypes.byref(nm), ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return a[:nm.value], b[:nm.value], d[:nm.value], size[:nm.value]


def linkage_files(files, method, ksize=21, algo="histosketch", metric="jaccard", csv_path=None, cut_distance=None, cut_csv_path=None,
                  threads=0, device=0, stats=None):
    """The directory form (hulk_linkage_files): dendrogram_files' loader, CSV ("merge,sketch_a,sketch_b,distance,similarity,size", one
    line per merge in the order performed) and cut (the clusters file of the merges with distance <= cut_distance: what
    cut_dendrogram gives), under the linkage `method`.  -> (ordering, a, b, d, size); ordering = the sorted unique paths."""
    _check_metric(metric)
    _check_algo(algo)
    _check_linkage(method)
    ordering = sorted(set(files))
    n = max(len(ordering), 1)
    a = np.zeros(n, dtype=np.uint32); b = np.zeros(n, dtype=np.uint32); d = np.zeros(n, dtype=np.float64); size = np.zeros(n, dtype=np.uint32)
    nm = ctypes.c_uint32(0)
    arr, n_paths = _paths(files)
    st = _lib.LinkageStats()
    _call_files(_lib.load().hulk_linkage_files, device, arr, n_paths, ksize, algo.encode(), metric.encode(), method.encode(), threads, _fs(csv_path),
                float("nan") if cut_distance is None else float(cut_distance), _fs(cut_csv_path),
                a.ctypes.data, b.ctypes.data, d.ctypes.data, size.ctypes.data, ctypes.byref(nm), ctypes.byref(st))
    if stats is not None:
        stats.update(_stats(st))
    return ordering, a[:nm.value], b[:nm.value], d[:nm.value], size[:nm.value]


def cut_dendrogram(n, a, b, d, max_distance):
    """The clusters of a dendrogram at a threshold, on the host: -> (labels uint32[n], n_clusters) — the components of the edges
    with d <= max_distance, labels[i] the smallest member of i's component: what cluster() gives at that max_distance."""
    n = int(n)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for x, y, h in zip(np.asarray(a).tolist(), np.asarray(b).tolist(), np.asarray(d, dtype=np.float64).tolist()):
        if not 0 <= x < n or not 0 <= y < n:
            raise ValueError("an edge outside the set")
        if h <= max_distance:
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)
    labels = np.array([find(i) for i in range(n)], dtype=np.uint32)
    return labels, int((labels == np.arange(n)).sum())


def linkage_matrix(n, a, b, d):
    """The dendrogram in the layout of scipy.cluster.hierarchy.linkage: an (n - 1) x 4 float64 array, row t = (id, id, distance,
    size) of merge t, ids < n the sketches, id n + t the cluster merge t created (the smaller id first).  The edges are taken in
    the order given, which is ascending for dendrogram()'s output.  ValueError when the forest is not one tree (n - 1 edges that
    join n sketches).  SciPy is not needed."""
    n = int(n)
    a = np.asarray(a).tolist(); b = np.asarray(b).tolist(); d = np.asarray(d, dtype=np.float64).tolist()
    if n < 1 or not len(a) == len(b) == len(d) == n - 1:
        raise ValueError(f"not one tree: {len(a)} edges for {n} sketches (a forest has no linkage matrix)")
    parent = list(range(n))
    ident = list(range(n))                                          # root -> the id of its cluster
    size = [1] * n

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    Z = np.zeros((n - 1, 4), dtype=np.float64)
    for t, (x, y, h) in enumerate(zip(a, b, d)):
        if not 0 <= x < n or not 0 <= y < n:
            raise ValueError("an edge outside the set")
        rx, ry = find(x), find(y)
        if rx == ry:
            raise ValueError("not one tree: an edge inside a cluster")
        lo, hi = min(rx, ry), max(rx, ry)
        Z[t] = (min(ident[rx], ident[ry]), max(ident[rx], ident[ry]), h, size[rx] + size[ry])
        parent[hi] = lo
        size[lo] = size[rx] + size[ry]
        ident[lo] = n + t
    return Z


def go_format_f2(v: float) -> str:
    """strconv.FormatFloat(v, 'f', 2, 64)"""
    if v != v:
        return "NaN"
    if v in (float("inf"), float("-inf")):
        return "+Inf" if v > 0 else "-Inf"
    return f"{v:.2f}"


def go_csv_field(f: str) -> str:
    """encoding/csv Writer: quote a field only when it needs it (fieldNeedsQuotes)."""
    need = f == "\\." or any(ch in f for ch in ',"\r\n') or (f != "" and f[0] in " \t")
    return '"' + f.replace('"', '""') + '"' if need else f


def find_sketch(data, ksize, algo, path):
    """HULKdata.FindSketch (sketchio.go:198-257) for histosketch signatures."""
    if algo not in AVAIL_ALGORITHMS:
        raise HulkError(-30, f"specified algorithm ({algo}) not found in the supplied sketch: {data.filename}\n")
    sigs = [hs for a, hs in data.signatures if a == algo]
    if not sigs:
        raise HulkError(-30, f"no sketches were produced using the {algo} algorithm in file: {data.filename}\n")
    hit = [hs for hs in sigs if hs.ksize == ksize]
    if len(hit) > 1:
        raise HulkError(-30, f"found {len(hit)} possible duplicate sketches in the supplied sketch file: {data.filename}\n")
    if not hit:
        raise HulkError(-30, f"specified k-mer size ({ksize}) not found in the supplied sketch file: {data.filename}\n")
    return hit[0]


def _paths(files):
    enc = [os.fsencode(f) for f in files]
    return (ctypes.c_char_p * max(len(enc), 1))(*enc), len(enc)


def load_sketches(files, ksize=21, algo="histosketch", threads=0):
    """LoadHULKdata + FindSketch for every file, in native code on `threads` host threads (hulk_load_sketches; no GPU needed):
    -> (ordering, mins[n][S], weights[n][S], banner labels), ordering = the sorted paths.  Raises HulkError with the reference's text."""
    L = _lib.load()
    arr, n = _paths(files)
    h = ctypes.c_void_p()
    _call_files(L.hulk_load_sketches, arr, n, ksize, algo.encode(), threads, ctypes.byref(h))
    try:
        cn, cs = ctypes.c_uint32(), ctypes.c_uint32()
        L.hulk_sketch_set_info(h, ctypes.byref(cn), ctypes.byref(cs))
        n, S = cn.value, cs.value
        mins = np.ctypeslib.as_array(ctypes.cast(L.hulk_sketch_set_mins(h), ctypes.POINTER(ctypes.c_uint64)), shape=(n * max(S, 1),))[:n * S].reshape(n, S).copy()
        weights = np.ctypeslib.as_array(ctypes.cast(L.hulk_sketch_set_weights(h), ctypes.POINTER(ctypes.c_double)), shape=(n * max(S, 1),))[:n * S].reshape(n, S).copy()
        ordering = [os.fsdecode(L.hulk_sketch_set_path(h, i)) for i in range(n)]
        banners = [L.hulk_sketch_set_banner(h, i).decode("utf-8", "replace") for i in range(n)]
    finally:
        L.hulk_sketch_set_free(h)
    return ordering, mins, weights, banners


def smash(sketch_dir, out_file, ksize=21, algo="histosketch", metric="jaccard", recursive=False, device=0,
          banner_matrix=False, stages=None, threads=0):
    """runSmash + makeMatrix (cmd/smash.go:60-226), native from the file names on (hulk_smash_files): the JSON files are parsed
    and MD5-verified on `threads` host threads, the N x N x S comparison runs on the GPU, the CSV is written by the library.
    Writes <out_file>.hulk-matrix.csv (and, banner_matrix, <out_file>.banner-matrix.csv: makeBannerMatrix, cmd/smash.go:229-261 —
    the reference iterates a Go map, here the sorted file order is used) and returns (ordering, distances).
    stages: a dict that receives the seconds of "load" (JSON + MD5 check), "matrix", "csv" and "kernel_ms"."""
    _check_metric(metric)
    _check_algo(algo)
    files = collect_jsons(sketch_dir, recursive)
    _make_parent_dir(out_file)
    L = _lib.load()
    arr, n = _paths(files)
    n_unique = len(set(files))
    dist = np.zeros((n_unique, n_unique), dtype=np.float64)
    st = _lib.SmashStats()
    _call_files(L.hulk_smash_files, device, arr, n, ksize, algo.encode(), metric.encode(), threads, os.fsencode(out_file + ".hulk-matrix.csv"),
                os.fsencode(out_file + ".banner-matrix.csv") if banner_matrix else None, dist.ctypes.data, ctypes.byref(st))
    if stages is not None:
        stages.update(load=st.seconds_load, matrix=st.seconds_matrix, csv=st.seconds_csv, kernel_ms=st.kernel_ms)
    return sorted(set(files)), dist


def smash_python(sketch_dir, out_file, ksize=21, algo="histosketch", metric="jaccard", recursive=False, device=0,
          banner_matrix=False, stages=None):
    """The same run with the load, the ordering and the CSV in Python (json + hashlib; the form `smash` had until round 6, kept as
    the comparator of the native one in tests/).  runSmash + makeMatrix: writes <out_file>.hulk-matrix.csv and returns (ordering, distances).
    banner_matrix: also <out_file>.banner-matrix.csv (makeBannerMatrix, cmd/smash.go:229-261): one line
    per sketch = its mins + the banner label; the reference iterates a Go map (random order), here the
    sorted file order is used.  stages: a dict that receives the seconds of "load" (JSON + MD5 check), "matrix", "csv"."""
    import time
    t_start = time.perf_counter()
    _check_metric(metric)
    _check_algo(algo)
    files = collect_jsons(sketch_dir, recursive)
    loaded = {}
    for f in files:
        try:
            loaded[f] = load_hulk_data(f)
        except ValueError as e:
            raise HulkError(-30, str(e))
    if len(loaded) < 2:
        raise HulkError(-30, f"{len(loaded)} sketches found in the supplied directory, HULK needs at least 2 to smash!\n")
    ordering = sorted(loaded)                                   # sort.Strings (byte order)
    sk = [find_sketch(loaded[f], ksize, algo, f) for f in ordering]
    size = len(sk[0].mins)
    for a in sk:
        if len(a.mins) != size:
            raise HulkError(-30, f"sketch length mismatch: {size} vs {len(a.mins)}\n")
    mins = np.stack([a.mins for a in sk])
    if algo == "histosketch":
        if metric == "bottomk":
            raise HulkError(-30, "bottomk is only supported for kmv sketches")
        weights = np.stack([a.weights for a in sk])
    elif metric == "weightedjaccard":                           # sketchio.go:287-293
        raise HulkError(-30, "weighted jaccard is only supported for histosketches")
    else:
        if metric == "bottomk" and algo != "kmv":
            raise HulkError(-30, "bottomk is only supported for kmv sketches")
        weights = np.zeros(mins.shape)                          # MinHash signatures carry no weights (khf.go:12-16)
    t_loaded = time.perf_counter()
    dist = distance_matrix(mins, weights, metric, device)
    t_matrix = time.perf_counter()
    _make_parent_dir(out_file)
    with open(out_file + ".hulk-matrix.csv", "w", encoding="utf-8", newline="") as fh:
        fh.write(",".join(go_csv_field(f) for f in ordering) + "\n")
        for row in dist:
            v = 100 - (row * 100)                                  # (elementwise IEEE double arithmetic: the Go expression)
            if np.isfinite(v).all():                               # FormatFloat(v, 'f', 2, 64) == "%.2f" for finite values
                fh.write(",".join(["%.2f" % x for x in v.tolist()]) + "\n")
            else:
                fh.write(",".join(go_format_f2(x) for x in v.tolist()) + "\n")
    if banner_matrix:
        with open(out_file + ".banner-matrix.csv", "w", encoding="utf-8", newline="") as fh:
            for f, a in zip(ordering, sk):
                fh.write(",".join([str(int(v)) for v in a.mins] + [go_csv_field(loaded[f].banner_label)]) + "\n")
    if stages is not None:
        stages.update(load=t_loaded - t_start, matrix=t_matrix - t_loaded, csv=time.perf_counter() - t_matrix)
    return ordering, dist
