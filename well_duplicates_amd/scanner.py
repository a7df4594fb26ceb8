"""Python face of the device scan path (thin: everything heavy is in libwelldup.so).

`Scanner` wraps one `wd_ctx` (one GPU).  `TileBatch` keeps the BCL planes and filter bytes
of a list of tiles resident in HBM in the layout the kernels like best: one slab
[tile][cycle][N padded to 256 B], so consecutive cycle planes of a tile are a constant
stride apart and every plane starts 256-byte aligned.
"""
from __future__ import annotations

import ctypes
import os
from typing import Callable, Iterable, List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._lib import MODE_EQ, MODE_HAMMING, MODE_LEVENSHTEIN, INVALID_TARGET  # noqa: F401

PLANE_ALIGN = 256


def compare_mode(edit_distance: int, hamming: bool):
    """Map the reference's -e / --hamming flags (count_well_duplicates.py:200, :258) to
    (mode, k).  -e 0 is string equality under either metric."""
    if edit_distance == 0:
        return MODE_EQ, 0
    return (MODE_HAMMING if hamming else MODE_LEVENSHTEIN), int(edit_distance)


def _raise(lib, ctx, rc: int, path: Optional[str] = None):
    """Raise what the reference would: the exception classes of include/welldup.h's table.
    `path` names the file a loader was reading (one of thousands per batch)."""
    detail = lib.wd_last_error(ctx).decode() if ctx else ""
    msg = "%s%s" % (lib.wd_strerror(rc).decode(), (": " + detail) if detail else "")
    if path is not None:
        msg = "%s: %s" % (msg, path)
    if rc == _lib.ERR_INDEX:
        raise IndexError(msg)            # bcl_direct_reader.py:186-192
    if rc == _lib.ERR_EMPTY_LEVEL:
        raise AssertionError(msg)        # count_well_duplicates.py:249
    if rc == _lib.ERR_ARG:
        raise ValueError(msg)
    if rc == _lib.ERR_NOMEM:
        raise MemoryError(msg)
    if rc == _lib.ERR_IO:
        raise FileNotFoundError(msg)      # bcl_direct_reader.py:207-216
    if rc == _lib.ERR_TRUNCATED:
        raise EOFError(msg)               # gzip.open(..).read() on a file that ends early (:208-209)
    if rc == _lib.ERR_CORRUPT:
        # ... on bad data: BadGzipFile when it is not a gzip file at all, else zlib.error
        import gzip
        import zlib
        magic = b""
        try:
            if path is not None and not path.endswith(".cbcl"):
                with open(path, "rb") as fh:
                    magic = fh.read(2)
        except OSError:
            pass
        if magic and magic != b"\x1f\x8b":
            raise gzip.BadGzipFile(msg)
        raise zlib.error(msg)
    if rc == _lib.ERR_FORMAT:
        raise AssertionError(msg)         # bcl_direct_reader.py:151, :236, :338
    raise RuntimeError(msg)


class Scanner:
    """One GPU context: resident targets + scan calls."""

    def __init__(self, device: int = -1):
        self._lib = _lib.load()
        self._ctx = self._lib.wd_create(device)
        if not self._ctx:
            rc = self._lib.wd_create_status()
            raise RuntimeError("wd_create(%d) failed: %s" % (device, self._lib.wd_strerror(rc).decode()))
        self.T = 0
        self.levels = 0
        self._owned = set()

    # ------------------------------------------------------------------ plumbing
    def _ck(self, rc: int):
        if rc != _lib.OK:
            _raise(self._lib, self._ctx, rc)

    def close(self, exiting: bool = False):
        """Destroys the context.  exiting=True: the process ends right after (the CLI's case) - the library
        then only waits for the device and leaves the freeing to the driver ("fast_exit", include/welldup.h)."""
        if self._ctx:
            if exiting:
                self._lib.wd_set_option(self._ctx, b"fast_exit", 1)
            else:
                for p in list(self._owned):
                    self._lib.wd_free(self._ctx, p)
            self._owned.clear()
            self._lib.wd_destroy(self._ctx)
            self._ctx = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        self._ck(self._lib.wd_set_option(self._ctx, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64()
        self._ck(self._lib.wd_get_option(self._ctx, name.encode(), ctypes.byref(v)))
        return v.value

    def set_stream(self, hip_stream: Optional[int]):
        self._ck(self._lib.wd_set_stream(self._ctx, ctypes.c_void_p(hip_stream or 0)))

    def synchronize(self):
        self._ck(self._lib.wd_synchronize(self._ctx))

    def malloc(self, nbytes: int) -> int:
        p = ctypes.c_void_p()
        self._ck(self._lib.wd_malloc(self._ctx, int(nbytes), ctypes.byref(p)))
        self._owned.add(p.value)
        return p.value

    def free(self, ptr: int):
        if ptr in self._owned:
            self._owned.discard(ptr)
            self._ck(self._lib.wd_free(self._ctx, ctypes.c_void_p(ptr)))

    def h2d(self, dst: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        self._ck(self._lib.wd_memcpy_h2d(self._ctx, ctypes.c_void_p(dst),
                                         arr.ctypes.data_as(ctypes.c_void_p), arr.nbytes))

    def d2h(self, src: int, nbytes: int, dtype=np.uint8) -> np.ndarray:
        out = np.empty(int(nbytes) // np.dtype(dtype).itemsize, dtype=dtype)
        self._ck(self._lib.wd_memcpy_d2h(self._ctx, out.ctypes.data_as(ctypes.c_void_p),
                                         ctypes.c_void_p(src), out.nbytes))
        return out

    def memset(self, dst: int, value: int, nbytes: int):
        self._ck(self._lib.wd_memset(self._ctx, ctypes.c_void_p(dst), value, int(nbytes)))

    # ------------------------------------------------------------------ targets
    def set_targets(self, centre, lvl_off, nbr):
        """CSR as AllTargets.to_csr(): centre[T], lvl_off[T, levels+1], nbr[P] (int32)."""
        centre = np.ascontiguousarray(centre, dtype=np.int32)
        lvl_off = np.ascontiguousarray(lvl_off, dtype=np.int32)
        nbr = np.ascontiguousarray(nbr, dtype=np.int32)
        if lvl_off.ndim != 2 or lvl_off.shape[0] != centre.shape[0]:
            raise ValueError("lvl_off must be [T, levels+1]")
        T, levels = centre.shape[0], lvl_off.shape[1] - 1
        if T and int(lvl_off[:, -1].max()) > nbr.shape[0]:
            raise ValueError("lvl_off points past the end of nbr")
        self._ck(self._lib.wd_set_targets(
            self._ctx, T, levels, centre.ctypes.data_as(ctypes.c_void_p),
            lvl_off.ctypes.data_as(ctypes.c_void_p), nbr.ctypes.data_as(ctypes.c_void_p)))
        self.T, self.levels = T, levels

    def targets_from_coords(self, x, y, centres=None, levels=5, max_dists=None):
        """Neighbour rings on the device (prepare_cluster_indexes.py:38-78 semantics) for the
        given centre wells, or for every well when `centres` is None.  The result becomes the
        scanner's targets; returns (T, P)."""
        from .cluster_indexes import max_dists_for
        x = np.ascontiguousarray(x, dtype=np.int32)
        y = np.ascontiguousarray(y, dtype=np.int32)
        md = np.ascontiguousarray(max_dists if max_dists is not None else max_dists_for(levels),
                                  dtype=np.int32)
        if md.shape[0] != levels + 1:
            raise ValueError("max_dists must hold levels + 1 radii")
        c = None if centres is None else np.ascontiguousarray(centres, dtype=np.int32)
        P = ctypes.c_int64()
        self._ck(self._lib.wd_targets_from_coords(
            self._ctx, x.ctypes.data_as(ctypes.c_void_p), y.ctypes.data_as(ctypes.c_void_p),
            x.shape[0], c.ctypes.data_as(ctypes.c_void_p) if c is not None else None,
            0 if c is None else c.shape[0], levels, md.ctypes.data_as(ctypes.c_void_p),
            ctypes.byref(P)))
        self.T = x.shape[0] if c is None else c.shape[0]
        self.levels = levels
        return self.T, P.value

    def get_targets(self):
        """Download the resident targets as (centre, lvl_off, nbr) int32 arrays."""
        T, lv, P = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        self._ck(self._lib.wd_targets_info(self._ctx, ctypes.byref(T), ctypes.byref(lv), ctypes.byref(P)))
        centre = np.zeros(T.value, dtype=np.int32)
        lvl_off = np.zeros((T.value, lv.value + 1), dtype=np.int32)
        nbr = np.zeros(P.value, dtype=np.int32)
        self._ck(self._lib.wd_get_targets(self._ctx, centre.ctypes.data_as(ctypes.c_void_p),
                                          lvl_off.ctypes.data_as(ctypes.c_void_p),
                                          nbr.ctypes.data_as(ctypes.c_void_p)))
        return centre, lvl_off, nbr

    # ------------------------------------------------------------------ scan
    @staticmethod
    def _tables(planes, filters, L):
        n_tiles = len(filters)
        flat = [int(p) for tile in planes for p in tile]
        if len(flat) != n_tiles * L:
            raise ValueError("planes must hold n_tiles x L pointers")
        pt = (ctypes.c_void_p * max(1, len(flat)))(*flat)
        ft = (ctypes.c_void_p * max(1, n_tiles))(*[int(f) for f in filters])
        return pt, ft

    def count_tiles(self, planes: Sequence[Sequence[int]], filters: Sequence[int], n_clusters: int,
                    mode: int, k: int, per_target: bool = False, tables=None, L=None):
        """Synchronous scan of n_tiles tiles.

        planes[i][c]: device address of tile i's c-th scanned cycle plane (N bytes);
        filters[i]: device address of its filter bytes.  Returns (blocks, per_target):
        blocks int64 [n_tiles, 1 + 5*levels] as documented in include/welldup.h;
        per_target uint32 [n_tiles, T, levels] or None.
        """
        n_tiles = len(filters)
        if L is None:
            L = len(planes[0]) if n_tiles else 0
        pt, ft = tables if tables is not None else self._tables(planes, filters, L)
        blocks = np.zeros((n_tiles, 1 + 5 * self.levels), dtype=np.int64)
        pto = np.zeros((n_tiles, self.T, self.levels), dtype=np.uint32) if per_target else None
        self._ck(self._lib.wd_count_tiles(
            self._ctx, n_tiles, L, mode, k, pt, ft, int(n_clusters),
            blocks.ctypes.data_as(ctypes.c_void_p),
            pto.ctypes.data_as(ctypes.c_void_p) if per_target else None))
        return blocks, pto

    def _workspace_bytes(self, fn, *args) -> int:
        b = ctypes.c_size_t()
        self._ck(fn(*[int(a) for a in args], ctypes.byref(b)))
        return b.value

    def _tile_call(self, planes, filters, labels, tables, L, row_cols: int, call):
        """What tile_dups and tile_near_dups share: the pointer tables, a zeroed int64 [n_tiles, row_cols], the label
        table (or None), then call(n_tiles, L, plane table, filter table, rows pointer, label table) -> rc."""
        n_tiles = len(filters)
        if L is None:
            L = len(planes[0]) if n_tiles else 0
        pt, ft = tables if tables is not None else self._tables(planes, filters, L)
        rows = np.zeros((n_tiles, row_cols), dtype=np.int64)
        lt = (ctypes.c_void_p * max(1, n_tiles))(*[int(p) for p in labels]) if labels is not None else None
        self._ck(call(n_tiles, L, pt, ft, rows.ctypes.data_as(ctypes.c_void_p), lt))
        return rows

    def dup_sets_workspace_bytes(self, n_clusters: int, n_tiles: int) -> int:
        """Device bytes wd_dup_sets needs as its workspace for n_tiles tiles of n_clusters wells."""
        return self._workspace_bytes(self._lib.wd_dup_sets_workspace, n_clusters, n_tiles)

    def dup_sets(self, planes: Sequence[Sequence[int]], filters: Sequence[int], n_clusters: int, mode: int, k: int,
                 workspace: int, workspace_bytes: int, labels: Optional[Sequence[int]] = None, edge_cap: int = 0,
                 tables=None, L=None):
        """The scan of count_tiles plus the duplicate sets of every tile (wd_dup_sets, include/welldup_sets.h);
        needs every well as a target.  labels: n_tiles device addresses of N uint32 each, or None.
        Returns (blocks [n_tiles, 1 + 5*levels], sets [n_tiles, 1 + 3*levels + 8], edges processed):
        a sets row is [PF wells, Sets[levels], InSets[levels], Redundant[levels], size bins 2..8, 9+]."""
        n_tiles = len(filters)
        if L is None:
            L = len(planes[0]) if n_tiles else 0
        pt, ft = tables if tables is not None else self._tables(planes, filters, L)
        blocks = np.zeros((n_tiles, 1 + 5 * self.levels), dtype=np.int64)
        sets = np.zeros((n_tiles, 1 + 3 * self.levels + _lib.DUPSET_SIZE_BINS), dtype=np.int64)
        lt = (ctypes.c_void_p * max(1, n_tiles))(*[int(p) for p in labels]) if labels is not None else None
        edges = ctypes.c_int64()
        self._ck(self._lib.wd_dup_sets(
            self._ctx, n_tiles, L, mode, k, pt, ft, int(n_clusters), ctypes.c_void_p(workspace), int(workspace_bytes),
            int(edge_cap), blocks.ctypes.data_as(ctypes.c_void_p), sets.ctypes.data_as(ctypes.c_void_p), lt,
            ctypes.byref(edges)))
        return blocks, sets, edges.value

    def tile_dups_workspace_bytes(self, n_clusters: int, n_tiles: int) -> int:
        """Device bytes wd_tile_dups needs as its workspace for n_tiles tiles of n_clusters wells."""
        return self._workspace_bytes(self._lib.wd_tile_dups_workspace, n_clusters, n_tiles)

    def tile_dups(self, planes: Sequence[Sequence[int]], filters: Sequence[int], n_clusters: int, workspace: int,
                  workspace_bytes: int, labels: Optional[Sequence[int]] = None, hash_bits: int = 0, tables=None, L=None):
        """The read classes of every tile (wd_tile_dups, include/welldup_tiledups.h): PF wells with equal reads
        wherever on the tile they lie; needs every well as a target.  labels: n_tiles device addresses of N
        uint32 each, or None.  Returns rows [n_tiles, 4 + 2*levels + 8]: [PF wells, Classes, InClasses,
        Redundant, Local[levels], RingWells[levels], size bins 2..8, 9+]."""
        return self._tile_call(
            planes, filters, labels, tables, L, 4 + 2 * self.levels + _lib.DUPSET_SIZE_BINS,
            lambda n_tiles, L, pt, ft, rows, lt: self._lib.wd_tile_dups(
                self._ctx, n_tiles, L, pt, ft, int(n_clusters), ctypes.c_void_p(workspace), int(workspace_bytes),
                int(hash_bits), rows, lt))

    def tile_near_dups_workspace_bytes(self, n_clusters: int, n_tiles: int, k: int) -> int:
        """Device bytes wd_tile_near_dups needs as its workspace for n_tiles tiles of n_clusters wells at distance k."""
        return self._workspace_bytes(self._lib.wd_tile_near_dups_workspace, n_clusters, n_tiles, k)

    def tile_near_dups(self, planes: Sequence[Sequence[int]], filters: Sequence[int], n_clusters: int, k: int,
                       workspace: int, workspace_bytes: int, labels: Optional[Sequence[int]] = None, hash_bits: int = 0,
                       pair_budget: int = 0, tables=None, L=None):
        """The near-duplicate clusters of every tile (wd_tile_near_dups, include/welldup_tilenear.h): PF wells
        linked by Hamming distance <= k wherever on the tile they lie; needs every well as a target.  labels:
        n_tiles device addresses of N uint32 each, or None.  Returns rows [n_tiles, 5 + 2*levels + 8]: [PF wells,
        Clusters, InClusters, Redundant, NearPairs, Local[levels], RingWells[levels], size bins 2..8, 9+].  A tile
        with more candidate pairs in a segment than pair_budget (0 = the default) raises RuntimeError."""
        return self._tile_call(
            planes, filters, labels, tables, L, 5 + 2 * self.levels + _lib.DUPSET_SIZE_BINS,
            lambda n_tiles, L, pt, ft, rows, lt: self._lib.wd_tile_near_dups(
                self._ctx, n_tiles, L, pt, ft, int(n_clusters), int(k), ctypes.c_void_p(workspace), int(workspace_bytes),
                int(hash_bits), int(pair_budget), rows, lt))

    def lane_dups_workspace_bytes(self, n_clusters: int, max_tiles: int, L: int) -> int:
        """Device bytes a LaneDups accumulator needs for max_tiles tiles of n_clusters wells and L cycles
        (wd_lane_dups_workspace; a lane of 2^32 - 1 wells or more raises RuntimeError)."""
        return self._workspace_bytes(self._lib.wd_lane_dups_workspace, n_clusters, max_tiles, L)

    def lane_near_scratch_bytes(self, n_clusters: int, max_tiles: int, L: int, k: int) -> int:
        """Device bytes LaneDups.finish(hamming=k) needs beside the accumulator's workspace
        (wd_lane_near_dups_scratch; 0 for k = 0)."""
        return self._workspace_bytes(self._lib.wd_lane_near_dups_scratch, n_clusters, max_tiles, L, k)

    def lane_index_workspace_bytes(self, n_clusters: int, max_tiles: int, I: int) -> int:
        """Device bytes the index part of a LaneDups accumulator needs for I index cycles
        (wd_lane_index_workspace; I outside 1..20 raises ValueError)."""
        return self._workspace_bytes(self._lib.wd_lane_index_workspace, n_clusters, max_tiles, I)

    def lane_mismatch_scratch_bytes(self, max_tiles: int, L: int) -> int:
        """Device bytes LaneDups.mismatches needs beside the accumulator's workspace (wd_lane_mismatch_scratch;
        it does not depend on the wells of a tile)."""
        return self._workspace_bytes(self._lib.wd_lane_mismatch_scratch, max_tiles, L)

    def lane_gc_scratch_bytes(self, max_tiles: int, L: int) -> int:
        """Device bytes LaneDups.gc needs beside the accumulator's workspace (wd_lane_gc_scratch: the counters per
        tile and the histogram per g; it does not depend on the wells of a tile)."""
        return self._workspace_bytes(self._lib.wd_lane_gc_scratch, max_tiles, L)


    def lane_adapter_scratch_bytes(self, max_tiles: int, L: int) -> int:
        """Device bytes LaneDups.adapter needs beside the accumulator's workspace (wd_lane_adapter_scratch: the
        counters per tile, the histogram per a, the tile indices and the search's table)."""
        return self._workspace_bytes(self._lib.wd_lane_adapter_scratch, max_tiles, L)
    def lane_consensus_scratch_bytes(self, max_tiles: int, n_clusters: int, L: int) -> int:
        """Device bytes LaneDups.consensus needs beside the accumulator's workspace (wd_lane_consensus_scratch: 8 bytes
        per well of the lane - where a family's members begin, and the member list with the family table - and the
        counters)."""
        return self._workspace_bytes(self._lib.wd_lane_consensus_scratch, max_tiles, n_clusters, L)

    def lane_umi_workspace_bytes(self, n_clusters: int, max_tiles: int, U: int) -> int:
        """Device bytes the UMI part of a lane's accumulator needs: 8 per well plus the pointer tables
        (wd_lane_umi_workspace; U outside 1..20 raises ValueError)."""
        return self._workspace_bytes(self._lib.wd_lane_umi_workspace, n_clusters, max_tiles, U)

    def lane_umi_scratch_bytes(self, max_tiles: int, n_clusters: int) -> int:
        """Device bytes LaneDups.umi needs beside the accumulator's workspace (wd_lane_umi_scratch: 8 bytes per well of
        the lane - where a family's range begins, the member list and the family table - plus the counters)."""
        return self._workspace_bytes(self._lib.wd_lane_umi_scratch, max_tiles, n_clusters)

    def lane_molecules_bytes(self, max_tiles: int, n_clusters: int) -> int:
        """Device bytes of the molecule region LaneDups.umi(molecules=True) fills (wd_lane_molecules_bytes: 8 bytes per
        well of the lane)."""
        return self._workspace_bytes(self._lib.wd_lane_molecules_bytes, max_tiles, n_clusters)

    def lane_keep_scratch_bytes(self, max_tiles: int, n_clusters: int) -> int:
        """Device bytes LaneDups.keep needs beside the accumulator's workspaces (wd_lane_keep_scratch: 10 bytes per well
        of the lane - the best of the family rooted there and the well's score - plus the counters, the tile indices and
        the mask pointers)."""
        return self._workspace_bytes(self._lib.wd_lane_keep_scratch, max_tiles, n_clusters)

    def lane_hops_scratch_bytes(self, max_tiles: int, M: int) -> int:
        """Device bytes LaneDups.hops needs beside the accumulator's workspaces for M listed keys
        (wd_lane_hops_scratch: the counters, the listing and the (M + 1)^2 cells of the matrix; it does not depend on
        the wells of a tile; M outside 0..1024 raises ValueError)."""
        return self._workspace_bytes(self._lib.wd_lane_hops_scratch, max_tiles, M)

    def lane_distance_scratch_bytes(self, n_clusters: int, max_tiles: int, matrix: bool = True) -> int:
        """Device bytes LaneDups.distances needs beside the accumulator's workspace (wd_lane_distance_scratch: the
        coordinates of a tile's wells, the counters, and with `matrix` TilePairs; more than 4096 tiles with the
        matrix raise RuntimeError)."""
        return self._workspace_bytes(self._lib.wd_lane_distance_scratch, n_clusters, max_tiles, int(bool(matrix)))

    def lane_qual_workspace_bytes(self, n_clusters: int, max_tiles: int, L: int) -> int:
        """Device bytes the quality part of a LaneDups accumulator needs (wd_lane_qual_workspace: a second packed
        array of the packed rows' size, and the QHist counters)."""
        return self._workspace_bytes(self._lib.wd_lane_qual_workspace, n_clusters, max_tiles, L)

    def lane_qual_scratch_bytes(self, max_tiles: int) -> int:
        """Device bytes LaneDups.qualities needs beside the accumulator's workspaces (wd_lane_qual_scratch; it
        depends on neither the wells of a tile nor the cycles)."""
        return self._workspace_bytes(self._lib.wd_lane_qual_scratch, max_tiles)

    def lane_top_scratch_bytes(self, n_clusters: int, max_tiles: int, L: int, n_top: int, cand_capacity: int = 0) -> int:
        """Device bytes LaneDups.top needs beside the accumulator's workspace (wd_lane_top_scratch: the histograms,
        cand_capacity candidate roots - 0: 65536, raised to n_top -, and per listed group a row of tile counts and its
        packed read; the wells of a tile take no part)."""
        return self._workspace_bytes(self._lib.wd_lane_top_scratch, n_clusters, max_tiles, L, n_top, cand_capacity)

    def lane_saturation_scratch_bytes(self, n_clusters: int, max_tiles: int, coords: bool = True) -> int:
        """Device bytes LaneDups.saturation needs beside the accumulator's workspace (wd_lane_saturation_scratch: a
        word per well of the lane, the counters, and with `coords` the coordinates of a tile's wells)."""
        return self._workspace_bytes(self._lib.wd_lane_saturation_scratch, n_clusters, max_tiles, int(bool(coords)))

    def scan_async(self, tables, n_tiles: int, L: int, n_clusters: int, mode: int, k: int,
                   out_tile_dev: int, out_per_target_dev: Optional[int] = None):
        pt, ft = tables
        self._ck(self._lib.wd_scan_async(
            self._ctx, n_tiles, L, mode, k, pt, ft, int(n_clusters),
            ctypes.c_void_p(out_tile_dev), ctypes.c_void_p(out_per_target_dev or 0)))

    def scan_status(self):
        self._ck(self._lib.wd_scan_status(self._ctx))

    # ------------------------------------------------------------------ ingest
    def load_bcl_gz(self, path: str, dst: int, n_clusters: int, well_stride: int = 1):
        """gunzip a .bcl.gz straight into device memory (thread-safe, releases the GIL);
        well_stride = 4 writes the plane into its byte lane of an interleaved group."""
        rc = self._lib.wd_load_bcl_gz_strided(self._ctx, os.fsencode(path), ctypes.c_void_p(dst), int(n_clusters),
                                              int(well_stride))
        if rc != _lib.OK:
            _raise(self._lib, None, rc, path)

    def load_bcl_gz_batch(self, paths: Sequence[str], dsts: Sequence[int], n_clusters: int, threads: int = 16,
                          missing_ok: bool = False, filters: Sequence = (), well_stride: int = 1,
                          tile_of: Optional[Sequence[int]] = None):
        """Many .bcl.gz files -> device planes, inflated on the GPU (wd_load_bcl_gz_batch: host threads
        only read the compressed files; one wave per file decodes).  Raises what load_bcl_gz raises
        for the first file that fails; with missing_ok the files that do not exist are returned
        (as indices) instead, for the caller to look for a .cbcl.  filters: [(path, dst)] of the
        tiles' .filter files, loaded in the same call (a missing one always raises)."""
        n_gz = len(paths)
        paths = list(paths) + [f[0] for f in filters]
        dsts = list(dsts) + [f[1] for f in filters]
        n = len(paths)
        enc = [os.fsencode(p) for p in paths]
        c_paths = (ctypes.c_char_p * max(1, n))(*enc)
        c_dsts = (ctypes.c_void_p * max(1, n))(*[int(d) for d in dsts])
        kinds = (ctypes.c_uint8 * max(1, n))(*([0] * n_gz + [1] * (n - n_gz)))
        rcs = (ctypes.c_int * max(1, n))()
        rc = self._lib.wd_load_tile_files_batch(self._ctx, n, c_paths, c_dsts, kinds, int(n_clusters), int(well_stride),
                                                int(threads), rcs)
        if rc != _lib.OK and not any(rcs[i] != _lib.OK for i in range(n)):
            _raise(self._lib, None, rc)         # the call itself failed (no memory, no thread, HIP), not a file
        missing = []
        # which failure is reported: the reference meets a tile's .filter before that tile's cycle files
        # (bcl_direct_reader.py:124-132, :195 before :200-216) and the tiles one after the other; with
        # `tile_of` (tile of every plane, then of every filter) that order is kept, without it the
        # filters come first
        if tile_of is not None:
            order = sorted(range(n), key=lambda i: (tile_of[i], i < n_gz, i))
        else:
            order = list(range(n_gz, n)) + list(range(n_gz))
        for i in order:
            if rcs[i] == _lib.OK:
                continue
            if rcs[i] == _lib.ERR_IO and missing_ok and i < n_gz:
                missing.append(i)
                continue
            _raise(self._lib, None, rcs[i], paths[i])
        missing.sort()
        return missing

    def load_filter(self, path: str, dst: int, n_clusters: int):
        rc = self._lib.wd_load_filter(self._ctx, os.fsencode(path), ctypes.c_void_p(dst), int(n_clusters))
        if rc != _lib.OK:
            _raise(self._lib, None, rc, path)

    def load_cbcl_tile(self, path: str, tile: int, filter_dev: int, n_clusters: int, dst: int, well_stride: int = 1):
        """One tile's block of a NovaSeq .cbcl file -> byte plane on the device (thread-safe); well_stride = 4:
        into its byte lane of an interleaved group (dst = TileBatch.plane_ptr of an interleaved batch)."""
        rc = self._lib.wd_load_cbcl_tile_strided(self._ctx, os.fsencode(path), int(tile), ctypes.c_void_p(filter_dev),
                                                 int(n_clusters), ctypes.c_void_p(dst), int(well_stride))
        if rc != _lib.OK:
            _raise(self._lib, None, rc, path)

    def load_cbcl_batch(self, entries: Sequence, n_clusters: int, threads: int = 16, well_stride: int = 1):
        """entries: [(cbcl path, tile number, filter pointer, plane pointer)] - the tiles' blocks are
        inflated on the GPU in one launch and expanded (wd_load_cbcl_batch); the filters must be
        loaded.  Raises what load_cbcl_tile raises for the first entry that fails."""
        n = len(entries)
        c_paths = (ctypes.c_char_p * max(1, n))(*[os.fsencode(e[0]) for e in entries])
        c_tiles = (ctypes.c_int * max(1, n))(*[int(e[1]) for e in entries])
        c_filt = (ctypes.c_void_p * max(1, n))(*[int(e[2]) for e in entries])
        c_dst = (ctypes.c_void_p * max(1, n))(*[int(e[3]) for e in entries])
        rcs = (ctypes.c_int * max(1, n))()
        rc = self._lib.wd_load_cbcl_batch_strided(self._ctx, n, c_paths, c_tiles, c_filt, c_dst, int(n_clusters),
                                                  int(well_stride), int(threads), rcs)
        for i in range(n):
            if rcs[i] != _lib.OK:
                _raise(self._lib, None, rcs[i], entries[i][0])
        if rc != _lib.OK:
            _raise(self._lib, None, rc)         # the call itself failed, not an entry

    def gather_wells(self, plane_ptrs: Sequence[int], idx, n_clusters: int) -> np.ndarray:
        """uint8 [len(idx), L]: bytes of the given wells over the L planes."""
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        L = len(plane_ptrs)
        out = np.zeros((idx.shape[0], L), dtype=np.uint8)
        tbl = (ctypes.c_void_p * max(1, L))(*[int(p) for p in plane_ptrs])
        self._ck(self._lib.wd_gather_wells(self._ctx, tbl, L, idx.ctypes.data_as(ctypes.c_void_p),
                                           idx.shape[0], int(n_clusters),
                                           out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def gather_wells_batch(self, tb: "TileBatch", tile: int, idx) -> np.ndarray:
        """gather_wells over every cycle of one tile of a TileBatch, in the batch's layout."""
        self.set_option("well_stride", tb.interleave)
        try:
            return self.gather_wells([tb.plane_ptr(tile, c) for c in range(tb.L)], idx, tb.N)
        finally:
            self.set_option("well_stride", 1)

    # ------------------------------------------------------------------ dup log / profile
    def hitlog_enable(self, capacity: int):
        self._ck(self._lib.wd_hitlog_enable(self._ctx, int(capacity)))

    def hitlog_fetch(self, max_records: int):
        """-> (records of the last scan as a structured array, total number found).  The count is read
        first, so the host buffer is as large as the records there are, not as the log could hold."""
        total = ctypes.c_int64()
        self._ck(self._lib.wd_hitlog_fetch(self._ctx, None, 0, ctypes.byref(total)))
        # (the library copies at most what the device log held: records beyond its capacity were counted,
        # not kept - the caller sees that in total > len(records))
        n = max(0, min(total.value, int(max_records), self.get_option("hitlog_capacity")))
        dt = np.dtype([("tile", "<i4"), ("target", "<i4"), ("slot", "<i4"), ("dist", "<i4")])
        recs = np.zeros(n, dtype=dt)
        if n:
            self._ck(self._lib.wd_hitlog_fetch(self._ctx, recs.ctypes.data_as(ctypes.c_void_p), n, ctypes.byref(total)))
        return recs, total.value

    def profile_get(self):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        self._ck(self._lib.wd_profile_get(self._ctx, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def profile_reset(self):
        self._ck(self._lib.wd_profile_reset(self._ctx))

    def stream_read_gbs(self, dev_ptr: int, nbytes: int, passes: int = 5) -> float:
        """GB/s of a kernel that only reads `nbytes` of device memory (wd_stream_read_probe): what this box's
        HBM gives a stream - the yardstick beside a scan kernel's rate."""
        ms = ctypes.c_double()
        self._ck(self._lib.wd_stream_read_probe(self._ctx, ctypes.c_void_p(dev_ptr), nbytes, passes, ctypes.byref(ms)))
        return nbytes / (ms.value * 1e-3) / 1e9

    def last_kernel(self) -> str:
        """Template name of the compare kernel the last scan launched (wd_last_kernel)."""
        return self._lib.wd_last_kernel(self._ctx).decode()

    # ------------------------------------------------------------------ multi-GPU
    def comm_unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(_lib.UNIQUE_ID_BYTES)
        rc = self._lib.wd_comm_unique_id(buf)
        if rc != _lib.OK:
            _raise(self._lib, None, rc)
        return buf.raw

    def comm_init(self, rank: int, world: int, unique_id: bytes):
        assert len(unique_id) == _lib.UNIQUE_ID_BYTES
        self._ck(self._lib.wd_comm_init(self._ctx, rank, world, unique_id))

    def allreduce_counts(self, buf_dev: int, n: int):
        self._ck(self._lib.wd_allreduce_counts(self._ctx, ctypes.c_void_p(buf_dev), n))

    def comm_destroy(self):
        self._ck(self._lib.wd_comm_destroy(self._ctx))

    # ------------------------------------------------------------------ synthetic data
    def _spec_c(self, spec, tile: int):
        return _lib.SynthSpecC(spec.seed, spec.n_clusters, spec.row, spec.nocall_per_64k,
                               spec.pass_per_64k, spec.plant_per_64k, int(spec.filter_noise),
                               int(int(tile) in tuple(int(t) for t in spec.dead_tiles)),
                               int(spec.plant_far), int(spec.qual_levels))

    def synth_plane(self, dst: int, spec, lane: int, tile: int, cycle: int):
        s = self._spec_c(spec, tile)
        self._ck(self._lib.wd_synth_plane(self._ctx, ctypes.c_void_p(dst), ctypes.byref(s),
                                          int(lane), int(tile), int(cycle)))

    def synth_filter(self, dst: int, spec, lane: int, tile: int):
        s = self._spec_c(spec, tile)
        self._ck(self._lib.wd_synth_filter(self._ctx, ctypes.c_void_p(dst), ctypes.byref(s),
                                           int(lane), int(tile)))


def _align256(v: int) -> int:
    return (v + 255) // 256 * 256


class _SidePart(NamedTuple):
    """What LaneDups knows of a side part `name` of its accumulator: it keeps the workspace in d_<name> with
    <name>_bytes, and what <name>_begin was given in the attribute `arg` (`none` before)."""
    name: str
    arg: str
    none: object
    conv: Callable          # the begin's argument as it is kept
    size: Callable          # (accumulator, the begin's argument) -> the workspace's bytes
    begin: Callable         # (library, handle, the argument, workspace, bytes) -> the return code of the begin entry
    add: str                # the add entry
    filters: bool           # the add takes the filter table too
    cycles: str             # the attribute that holds the cycles a TileBatch given to the add must have
    phrase: str             # what the shape error calls them


_SIDE_PARTS = {p.name: p for p in (
    _SidePart("index", "I", 0, int, lambda ld, I: ld.sc.lane_index_workspace_bytes(ld.N, ld.max_tiles, I),
              lambda lib, h, I, ws, n: lib.wd_lane_index_begin(h, I, ws, n), "wd_lane_index_add", False, "I", "index cycles"),
    _SidePart("qual", "qual_edges", None, lambda e: [int(v) for v in e], lambda ld, e: ld.sc.lane_qual_workspace_bytes(ld.N, ld.max_tiles, ld.L),
              lambda lib, h, e, ws, n: lib.wd_lane_qual_begin(h, len(e), (ctypes.c_int * max(1, len(e)))(*e), ws, n),
              "wd_lane_qual_add", True, "L", "cycles"),
    _SidePart("umi", "U", 0, int, lambda ld, U: ld.sc.lane_umi_workspace_bytes(ld.N, ld.max_tiles, U),
              lambda lib, h, U, ws, n: lib.wd_lane_umi_begin(h, U, ws, n), "wd_lane_umi_add", False, "U", "UMI cycles"))}


class LaneDups:
    """The read classes across all tiles of a lane (include/welldup_lanedups.h): an accumulator the batches of
    a lane are fed to one after the other.  It owns its workspace: a packed copy of every read and the lane's
    table, so a batch's planes may be reused as soon as `add` returns."""

    def __init__(self, scanner: Scanner, n_clusters: int, max_tiles: int, L: int, hash_bits: int = 0):
        self.sc = scanner
        self.N, self.max_tiles, self.L, self.hash_bits = int(n_clusters), int(max_tiles), int(L), int(hash_bits)
        self.ws_bytes = scanner.lane_dups_workspace_bytes(self.N, self.max_tiles, self.L)
        self.d_ws = scanner.malloc(self.ws_bytes)
        self.d_labels = self.d_near_labels = 0
        for part in _SIDE_PARTS.values():                # d_index, index_bytes, I; d_qual, qual_bytes, qual_edges; d_umi, umi_bytes, U
            self._part_set(part, 0, 0, part.none)
        self.index_listed = 0
        self.d_mol, self.mol_bytes = 0, 0                # the molecule region (umi(molecules=True))
        self.refused = None
        self.added = []                                  # the tile indices given to add, in that order
        self._h = None
        try:
            self._begin(self.d_ws, self.ws_bytes)
        except Exception:
            self.close()
            raise

    def _begin(self, workspace: int, workspace_bytes: int):
        h = ctypes.c_void_p()
        self.sc._ck(self.sc._lib.wd_lane_dups_begin(self.sc._ctx, self.N, self.max_tiles, self.L, ctypes.c_void_p(workspace),
                                                    int(workspace_bytes), self.hash_bits, ctypes.byref(h)))
        self._h = h

    def restart(self):
        """Drops what has been added and begins another lane of the same shape in the same workspace."""
        self._end()
        self.added = []
        self._begin(self.d_ws, self.ws_bytes)
        for part in _SIDE_PARTS.values():
            if getattr(self, part.arg) != part.none:
                self._part_rebegin(part)

    # ---- the side parts: one body each for begin, begin again after restart(), add and the feeding of an add entry
    def _part_set(self, part: _SidePart, ptr: int, nbytes: int, arg):
        setattr(self, "d_" + part.name, ptr)
        setattr(self, part.name + "_bytes", nbytes)
        setattr(self, part.arg, arg)

    def _part_begin(self, part: _SidePart, arg):
        """Allocates the part's workspace and begins it; a begin that fails leaves the accumulator without the part."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        if getattr(self, part.arg) != part.none:
            raise ValueError("%s_begin is called once" % part.name)
        arg = part.conv(arg)
        nbytes = part.size(self, arg)
        self._part_set(part, self.sc.malloc(max(1, nbytes)), nbytes, arg)
        try:
            self._part_rebegin(part)
        except Exception:
            self.sc.free(getattr(self, "d_" + part.name))
            self._part_set(part, 0, 0, part.none)
            raise

    def _part_rebegin(self, part: _SidePart):
        self.sc._ck(part.begin(self.sc._lib, self._h, getattr(self, part.arg), ctypes.c_void_p(getattr(self, "d_" + part.name)),
                               getattr(self, part.name + "_bytes")))

    def _part_add(self, part: _SidePart, tables, tile_indices: Sequence[int], well_stride: int):
        if self._h is None:
            raise ValueError("the accumulator is closed")
        idx = [int(t) for t in tile_indices]
        cycles = getattr(self, part.cycles)
        if isinstance(tables, TileBatch):
            tb = tables
            if len(idx) != tb.n_tiles or tb.L != cycles or tb.N != self.N:
                raise ValueError("the batch has %d tiles of %d wells and %d cycles; %d indices for a lane of %d wells "
                                 "and %d %s" % (tb.n_tiles, tb.N, tb.L, len(idx), self.N, cycles, part.phrase))
            tables, well_stride = tb.tables, tb.interleave
        if not part.filters:
            tables = tables[:1]
            if cycles and len(tables[0]) < len(idx) * cycles:
                raise ValueError("the plane table must hold n_tiles x %s pointers" % part.cycles)
        self._feed(part.add, idx, tables, well_stride)

    def _feed(self, entry: str, idx: Sequence[int], tables, well_stride: int):
        """An add entry of the library on the tiles idx, under well_stride - which is 1 again afterwards, whatever happened."""
        ti = (ctypes.c_int * max(1, len(idx)))(*idx)
        self.sc.set_option("well_stride", well_stride)
        try:
            self.sc._ck(getattr(self.sc._lib, entry)(self._h, len(idx), ti, *tables))
        finally:
            self.sc.set_option("well_stride", 1)

    def _key_array(self, d_ws: int, cycles: int, front: int) -> np.ndarray:
        """The key array of a key part's workspace: behind `front` bytes, the plane pointers and the tile indices."""
        at = front + _align256(8 * self.max_tiles * cycles) + _align256(4 * self.max_tiles)
        return self.sc.d2h(d_ws + at, 8 * self.N * self.max_tiles, np.uint64)

    def _with_scratch(self, nbytes: int, call):
        """call(scratch pointer, nbytes) -> a return code, checked; the scratch lives for the call."""
        d_scratch = self.sc.malloc(max(1, nbytes))
        try:
            self.sc._ck(call(ctypes.c_void_p(d_scratch), nbytes))
        finally:
            self.sc.free(d_scratch)

    def _coords(self, x, y):
        """x, y of a tile's N wells, each 0 .. 2^24 - 1 -> contiguous int32 arrays; ValueError names the first
        well that is out of range."""
        xs, ys = (np.asarray(v) for v in (x, y))
        if xs.shape != (self.N,) or ys.shape != (self.N,):
            raise ValueError("x and y hold a coordinate per well of a tile: %d each" % self.N)
        for v in (xs, ys):                               # (what int32 cannot hold is out of range as well)
            if v.size and (int(v.min()) < 0 or int(v.max()) > _lib.LANEDISTANCE_MAX_COORD):
                w = int(np.flatnonzero((v < 0) | (v > _lib.LANEDISTANCE_MAX_COORD))[0])
                raise ValueError("well %d lies at (%d, %d), outside 0..%d" % (w, xs[w], ys[w], _lib.LANEDISTANCE_MAX_COORD))
        return np.ascontiguousarray(xs, dtype=np.int32), np.ascontiguousarray(ys, dtype=np.int32)

    # ---- the lane's reported base quality against its copies (include/welldup_lanequality.h)
    def qual_begin(self, edges: Sequence[int]):
        """Gives the lane a quality part before the first add: edges are the bins' lower edges (1..8 of them,
        ascending from 0, at most 63).  The accumulator owns and frees its workspace."""
        self._part_begin(_SIDE_PARTS["qual"], edges)

    def qual_add(self, tables, tile_indices: Sequence[int], well_stride: int = 1):
        """Packs the qualities of resident tiles and counts QHist over their PF wells.  tables: the TileBatch `add`
        takes, or the ctypes pointer tables Scanner._tables makes (planes n x L, filters n); tile_indices as `add`
        takes them.  Independent of `add` in order and batching."""
        self._part_add(_SIDE_PARTS["qual"], tables, tile_indices, well_stride)

    def qualities(self, max_d: int):
        """After finish(), any number of times, before or after index_finish, mismatches and distances
        (wd_lane_qualities): every redundant well against its root under the labels the finish left, cycle by cycle,
        by the quality bins of the two.
        -> (lane row int64 [4]: [Pairs, Profiled, Observations, Mismatches], tile rows int64 [max_tiles, 4]: the same
        by the member's tile, qhist int64 [64]: the PF observations of the lane by raw quality, obs and mis int64
        [8, 8]: [root's bin][member's bin] over the pairs with d <= max_d, all cycles and those where the bases
        differ).  The scratch is allocated for the call and released.  max_d outside 0..7, a call before a successful
        finish or without qual_begin, or a tile that has reads but no qualities (or the reverse) raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        lane_row = np.zeros(_lib.LANEQUALITY_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEQUALITY_TILE_COLS), dtype=np.int64)
        qhist = np.zeros(_lib.LANEQUALITY_VALUES, dtype=np.int64)
        obs = np.zeros((_lib.LANEQUALITY_MAX_BINS, _lib.LANEQUALITY_MAX_BINS), dtype=np.int64)
        mis = np.zeros_like(obs)
        self._with_scratch(self.sc.lane_qual_scratch_bytes(self.max_tiles),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_qualities(
                               self._h, int(max_d), d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                               tile_rows.ctypes.data_as(ctypes.c_void_p), qhist.ctypes.data_as(ctypes.c_void_p),
                               obs.ctypes.data_as(ctypes.c_void_p), mis.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows, qhist, obs, mis

    # ---- the lane's duplication per index read (include/welldup_laneindex.h)
    def index_begin(self, I: int):
        """Gives the lane an index part of I cycles (1..20), before any finish; the accumulator owns and frees its
        workspace."""
        self._part_begin(_SIDE_PARTS["index"], I)

    def index_add(self, tables, tile_indices: Sequence[int], well_stride: int = 1):
        """Packs the index keys of resident tiles.  tables: a TileBatch of the I index cycles, or the ctypes pointer
        tables Scanner._tables makes (the planes n x I; the filters are not looked at); tile_indices as `add`
        takes them.  Independent of `add` in order and batching."""
        self._part_add(_SIDE_PARTS["index"], tables, tile_indices, well_stride)

    def index_keys(self) -> np.ndarray:
        """uint64 [max_tiles * N]: the index key of every well that got index planes (the key array of the index
        workspace; it lies where include/welldup_laneindex.h's arithmetic puts it: behind the counters, the plane
        pointers and the tile indices)."""
        return self._key_array(self.d_index, self.I, 4096 + 4096 + 256)

    def index_finish(self, min_pf: int = 1, cap: int = 1 << 16):
        """After finish(), any number of times.  -> (lane index row int64 [5]: [Groups, Listed, GroupSpans,
        MixedClasses, MixedWells], Other row int64 [5], group rows int64 [listed, 5]: [PF, InLane, InGroup,
        GroupRedundant, Mixed], keys uint64 [listed]), the groups of at least min_pf PF wells sorted by (-PF, key).
        More than cap such groups raise RuntimeError; `index_listed` then holds their number."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        cap = int(cap)
        lane_row = np.zeros(_lib.LANEINDEX_LANE_COLS, dtype=np.int64)
        other = np.zeros(_lib.LANEINDEX_GROUP_COLS, dtype=np.int64)
        rows = np.zeros((max(cap, 0), _lib.LANEINDEX_GROUP_COLS), dtype=np.int64)
        keys = np.zeros(max(cap, 0), dtype=np.uint64)
        n = ctypes.c_int64(0)
        rc = self.sc._lib.wd_lane_index_finish(self._h, int(min_pf), cap, lane_row.ctypes.data_as(ctypes.c_void_p),
                                               other.ctypes.data_as(ctypes.c_void_p),
                                               rows.ctypes.data_as(ctypes.c_void_p) if cap > 0 else None,
                                               keys.ctypes.data_as(ctypes.c_void_p) if cap > 0 else None, ctypes.byref(n))
        self.index_listed = n.value
        self.sc._ck(rc)
        rows, keys = rows[:n.value], keys[:n.value]
        order = np.lexsort((keys, -rows[:, 0]))
        return lane_row, other, rows[order], keys[order]

    # ---- the lane's duplicates split by molecular identifier (include/welldup_laneumi.h)
    def umi_begin(self, U: int):
        """Gives the lane a UMI part of U cycles (1..20), before any finish; the accumulator owns and frees its
        workspace.  A lane may carry an index part and a UMI part at once."""
        self._part_begin(_SIDE_PARTS["umi"], U)

    def umi_add(self, tables, tile_indices: Sequence[int], well_stride: int = 1):
        """Packs the UMI reads of resident tiles.  tables: a TileBatch of the U UMI cycles, or the ctypes pointer
        tables Scanner._tables makes (the planes n x U; the filters are not looked at); tile_indices as `add`
        takes them.  Independent of `add` in order and batching."""
        self._part_add(_SIDE_PARTS["umi"], tables, tile_indices, well_stride)

    def umi_keys(self) -> np.ndarray:
        """uint64 [max_tiles * N]: the UMI read of every well that got UMI planes, packed as index_keys packs an
        index read (the key array of the UMI workspace; it lies where include/welldup_laneumi.h's arithmetic puts it:
        behind the plane pointers and the tile indices)."""
        return self._key_array(self.d_umi, self.U, 0)

    def umi(self, max_e: int = 0, max_family: int = 256, molecules: bool = False):
        """After finish() of a lane with a UMI part, any number of times, before or after every other pass
        (wd_lane_umi, include/welldup_laneumi.h): the wells of every family of 2 .. max_family wells under the labels
        the finish left are grouped by their UMI read - a molecule is a connected component under "at most max_e UMI
        cycles differ" -, a larger family is counted and not looked into.
        -> (lane row int64 [27]: [Wells, UmiRedundant, Lone, Families, Molecules, DistinctUmis, SplitFamilies,
        SplitWells, WithN, LargeFamilies, LargeWells, MolPerFamily[8], MoleculeSize[8]], the histograms in bins of 1, 2,
        3, 4, 5-8, 9-16, 17-64 and 65 or more; tile rows int64 [max_tiles, 3]: [Wells, UmiRedundant, Lone] by the well's
        own tile).  The scratch is allocated for the call and released.  max_e outside 0..3, max_family outside 2..1024,
        a lane without a UMI part, a tile that has reads but no UMI planes (or the reverse) or a call before a
        successful finish raises ValueError.
        With `molecules` the same rows come from wd_lane_umi_molecules (include/welldup_lanemolecules.h), which also
        writes every well's molecule into a region the accumulator owns - allocated on the first such call, freed by
        close() -: what keep(by_molecule=True) then reads and umi_molecules() downloads."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        lane_row = np.zeros(_lib.LANEUMI_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEUMI_TILE_COLS), dtype=np.int64)
        if molecules:
            if not self.d_mol:
                self.mol_bytes = self.sc.lane_molecules_bytes(self.max_tiles, self.N)
                self.d_mol = self.sc.malloc(max(1, self.mol_bytes))
            self._with_scratch(self.sc.lane_umi_scratch_bytes(self.max_tiles, self.N),
                               lambda d_scratch, sbytes: self.sc._lib.wd_lane_umi_molecules(
                                   self._h, int(max_e), int(max_family), d_scratch, sbytes,
                                   lane_row.ctypes.data_as(ctypes.c_void_p), tile_rows.ctypes.data_as(ctypes.c_void_p),
                                   ctypes.c_void_p(self.d_mol), self.mol_bytes))
            return lane_row, tile_rows
        self._with_scratch(self.sc.lane_umi_scratch_bytes(self.max_tiles, self.N),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_umi(
                               self._h, int(max_e), int(max_family), d_scratch, sbytes,
                               lane_row.ctypes.data_as(ctypes.c_void_p), tile_rows.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows

    def molecule_part(self):
        """-> (max_e, max_family) of the umi(molecules=True) whose molecules keep(by_molecule=True) would read now, or
        None: there has been none since the finish, or the last one failed (wd_lane_molecules_part)."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        e, mf = ctypes.c_int(), ctypes.c_int()
        if self.sc._lib.wd_lane_molecules_part(self._h, ctypes.byref(e), ctypes.byref(mf)) != _lib.OK:
            return None
        return e.value, mf.value

    def umi_molecules(self):
        """-> (mol, molmem), uint32 [max_tiles, N] each: what the last umi(molecules=True) wrote (the two arrays of
        include/welldup_lanemolecules.h, molmem 4 * max_tiles * N bytes, rounded up to 256, behind mol).  ValueError
        before the first such call."""
        if not self.d_mol:
            raise ValueError("umi_molecules comes after umi(molecules=True)")
        wells = self.max_tiles * self.N
        at = _align256(4 * wells)
        shape = (self.max_tiles, self.N)
        if not wells:
            return np.zeros(shape, dtype=np.uint32), np.zeros(shape, dtype=np.uint32)
        return (self.sc.d2h(self.d_mol, 4 * wells, np.uint32).reshape(shape),
                self.sc.d2h(self.d_mol + at, 4 * wells, np.uint32).reshape(shape))

    def add(self, tb: "TileBatch", tile_indices: Sequence[int]):
        """Adds the tiles of a resident batch (a plane per cycle); tile_indices[i]: slot i's number in the lane,
        0 .. max_tiles - 1, each used once.  A bad index, the interleaved layout or a call after finish raises
        ValueError and changes nothing."""
        idx = [int(t) for t in tile_indices]
        if len(idx) != tb.n_tiles or tb.L != self.L or tb.N != self.N:
            raise ValueError("the batch has %d tiles of %d wells and %d cycles; %d indices for a lane of %d wells and "
                             "%d cycles" % (tb.n_tiles, tb.N, tb.L, len(idx), self.N, self.L))
        self.add_tables(idx, tb.tables, well_stride=tb.interleave)

    def add_tables(self, tile_indices: Sequence[int], tables, well_stride: int = 1):
        """add() from the ctypes pointer tables Scanner._tables makes (planes n x L, filters n)."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        self._feed("wd_lane_dups_add", tile_indices, tables, well_stride)
        self.added.extend(int(t) for t in tile_indices)

    def _label_table(self, attr: str):
        lbl_bytes = 4 * self.N * self.max_tiles
        if not getattr(self, attr):
            setattr(self, attr, self.sc.malloc(max(1, lbl_bytes)))
        base = getattr(self, attr)
        return (ctypes.c_void_p * max(1, self.max_tiles))(*[base + 4 * self.N * i for i in range(self.max_tiles)])

    def finish(self, labels: bool = False, hamming: int = 0, pair_budget: int = 0):
        """Once.  -> (lane row int64 [14]: [PF, Classes, InClasses, Redundant, CrossTileClasses, TileSpans, size
        bins 2..8, 9+], tile rows int64 [max_tiles, 5]: [PF, InLane, InTile, TileRedundant, LaneRedundant],
        labels uint32 [max_tiles, N] or None).
        With hamming = K > 0 (wd_lane_near_dups_finish, include/welldup_lanenear.h) three more follow, for the
        clusters at Hamming distance <= K: near lane row int64 [15] (NearPairs before the size bins), near tile rows
        and near labels.  The scratch is allocated for the call and released.  A lane with more candidate pairs in
        a segment than pair_budget (0 = the default) raises RuntimeError: `refused` then holds the equality
        results, which are valid, and finish may be called again."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        if hamming == 0 and pair_budget:
            raise ValueError("a pair budget needs hamming > 0")
        lane_row = np.zeros(_lib.LANEDUPS_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEDUPS_TILE_COLS), dtype=np.int64)
        lbl_bytes = 4 * self.N * self.max_tiles
        lt = self._label_table("d_labels") if labels else None
        fetch = lambda ptr: self.sc.d2h(ptr, lbl_bytes, np.uint32).reshape(self.max_tiles, self.N) if labels else None
        if hamming == 0:
            self.sc._ck(self.sc._lib.wd_lane_dups_finish(self._h, lane_row.ctypes.data_as(ctypes.c_void_p),
                                                         tile_rows.ctypes.data_as(ctypes.c_void_p), lt))
            return lane_row, tile_rows, fetch(self.d_labels)
        near_lane = np.zeros(_lib.LANENEAR_LANE_COLS, dtype=np.int64)
        near_tiles = np.zeros((self.max_tiles, _lib.LANEDUPS_TILE_COLS), dtype=np.int64)
        nlt = self._label_table("d_near_labels") if labels else None
        self.refused = None
        sbytes = self.sc.lane_near_scratch_bytes(self.N, self.max_tiles, self.L, hamming)     # (a bad K raises here)
        d_scratch = self.sc.malloc(max(1, sbytes))
        try:
            rc = self.sc._lib.wd_lane_near_dups_finish(
                self._h, int(hamming), ctypes.c_void_p(d_scratch), sbytes, int(pair_budget),
                lane_row.ctypes.data_as(ctypes.c_void_p), tile_rows.ctypes.data_as(ctypes.c_void_p), lt,
                near_lane.ctypes.data_as(ctypes.c_void_p), near_tiles.ctypes.data_as(ctypes.c_void_p), nlt)
            if rc == _lib.ERR_UNSUPPORTED:
                self.refused = (lane_row, tile_rows, fetch(self.d_labels))
            self.sc._ck(rc)
        finally:
            self.sc.free(d_scratch)
        return lane_row, tile_rows, fetch(self.d_labels), near_lane, near_tiles, fetch(self.d_near_labels)

    def mismatches(self, max_d: int):
        """After finish(), any number of times, before or after index_finish (wd_lane_mismatches,
        include/welldup_lanemismatch.h): every redundant well against its root under the labels the finish left.
        -> (lane row int64 [13]: [Pairs, Profiled, Mismatches, WithN, Dist d = 0..7 and >= 8], tile rows int64
        [max_tiles, 4]: [Pairs, Profiled, Mismatches, WithN] by the member's tile, sub int64 [L, 5, 5]:
        [cycle][root's code][member's code] over the pairs with d <= max_d).  The scratch is allocated for the
        call and released.  max_d outside 0..7 or a call before a successful finish raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        lane_row = np.zeros(_lib.LANEMISMATCH_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEMISMATCH_TILE_COLS), dtype=np.int64)
        sub = np.zeros((self.L, 5, 5), dtype=np.int64)
        self._with_scratch(self.sc.lane_mismatch_scratch_bytes(self.max_tiles, self.L),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_mismatches(
                               self._h, int(max_d), d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                               tile_rows.ctypes.data_as(ctypes.c_void_p), sub.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows, sub

    def gc(self, max_n: int = 0):
        """After finish(), any number of times, before or after every other pass (wd_lane_gc,
        include/welldup_lanegc.h): every PF well by the GC of its own read - g, its cycles that read C or G - and by
        what it is under the labels the finish left: a lone read, the first well of a group, or a copy.  A well with
        more than max_n no-calls is counted by population only.
        -> (lane row int64 [8]: [PF, Single, Roots, Copies, SkipSingle, SkipRoots, SkipCopies, SkipFamilyWells], tile
        rows int64 [max_tiles, 5]: [PF, Counted, GC, CopiesCounted, CopiesGC] by the well's own tile, hist int64
        [L + 1, 4]: [g][Single, Roots, Copies, FamilyWells], FamilyWells the groups' wells by the root's g).  The
        scratch is allocated for the call and released.  max_n outside 0..L or a call before a successful finish
        raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        lane_row = np.zeros(_lib.LANEGC_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEGC_TILE_COLS), dtype=np.int64)
        hist = np.zeros((self.L + 1, _lib.LANEGC_HIST_COLS), dtype=np.int64)
        self._with_scratch(self.sc.lane_gc_scratch_bytes(self.max_tiles, self.L),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_gc(
                               self._h, int(max_n), d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                               tile_rows.ctypes.data_as(ctypes.c_void_p), hist.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows, hist

    def adapter(self, codes, max_e: int = 1, min_overlap: int = 8):
        """After finish(), any number of times, before or after every other pass (wd_lane_adapter,
        include/welldup_laneadapter.h): every PF well by a, the first position at which its own read matches the
        adapter - codes, 8..32 values 0..3 (A C G T) - with at most max_e mismatches at full overlap, fewer in
        proportion where only min_overlap or more of the adapter's bases fit before the read's end, and by what it is
        under the labels the finish left: a lone read, the first well of a group, or a copy.  a = L: no adapter.
        -> (lane row int64 [10]: [PF, Single, Roots, Copies, AdSingle, AdRoots, AdCopies, AdFamilyWells, Inexact,
        Partial], tile rows int64 [max_tiles, 5]: [PF, Adapter, Copies, CopiesAdapter, SumA] by the well's own tile,
        hist int64 [L + 1, 4]: [a][Single, Roots, Copies, FamilyWells], FamilyWells the groups' wells by the root's
        a).  The scratch is allocated for the call and released.  An adapter, max_e or min_overlap out of range
        (min_overlap is 3..min(m, L)) or a call before a successful finish raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        codes = np.asarray(codes).reshape(-1)
        if codes.size and not (0 <= int(codes.min()) and int(codes.max()) <= 3):
            raise ValueError("an adapter's codes are 0..3 (A C G T)")
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        lane_row = np.zeros(_lib.LANEADAPTER_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEADAPTER_TILE_COLS), dtype=np.int64)
        hist = np.zeros((self.L + 1, _lib.LANEADAPTER_HIST_COLS), dtype=np.int64)
        self._with_scratch(self.sc.lane_adapter_scratch_bytes(self.max_tiles, self.L),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_adapter(
                               self._h, codes.ctypes.data_as(ctypes.c_void_p), int(codes.size), int(max_e),
                               int(min_overlap), d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                               tile_rows.ctypes.data_as(ctypes.c_void_p), hist.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows, hist

    def keep(self, min_q: int = _lib.LANEKEEP_DEFAULT_MIN_Q, masks: bool = False, by_molecule: bool = False):
        """After finish(), any number of times, before or after every other pass, on an accumulator with a quality part
        (wd_lane_keep, include/welldup_lanekeep.h): of every family - a class, or a cluster under a near finish - the
        well with the largest score is kept, the smallest id among equals, and the others are dropped; a well's score
        is the sum over its cycles of its quality bin's lower edge where that is at least min_q.
        -> (lane row int64 [17]: [PF, Kept, Dropped, MovedIn, SumKept, SumDropped, Families, Moved, SumRoots, GainBins
        x 8], tile rows int64 [max_tiles, 6]: the first six by the well's own tile), and with `masks` a third: {tile
        index: uint8 [N], 1 for a kept well and 0 for any other} for every tile that was added.  The scratch is
        allocated for the call and released.  min_q outside 0..63, a call before a successful finish or without
        qual_begin, or a tile that has reads but no qualities (or the reverse) raises ValueError.
        by_molecule: one well per UMI molecule, not per family (wd_lane_keep_molecules,
        include/welldup_lanemolecules.h): the molecules are those of the last umi(molecules=True) since the finish;
        without one ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        if by_molecule and not self.d_mol:
            raise ValueError("keep(by_molecule=True) comes after umi(molecules=True)")
        entry = self.sc._lib.wd_lane_keep_molecules if by_molecule else self.sc._lib.wd_lane_keep
        lane_row = np.zeros(_lib.LANEKEEP_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEKEEP_TILE_COLS), dtype=np.int64)
        tiles = sorted(self.added) if masks else []
        d_masks = self.sc.malloc(max(1, len(tiles) * self.N)) if tiles else 0
        try:
            table = None
            if tiles:
                ptrs = [None] * self.max_tiles
                for i, t in enumerate(tiles):
                    ptrs[t] = d_masks + i * self.N
                table = (ctypes.c_void_p * self.max_tiles)(*ptrs)
            self._with_scratch(self.sc.lane_keep_scratch_bytes(self.max_tiles, self.N),
                               lambda d_scratch, sbytes: entry(
                                   self._h, int(min_q), d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                                   tile_rows.ctypes.data_as(ctypes.c_void_p), table))
            if not masks:
                return lane_row, tile_rows
            out = {}
            if tiles and self.N:
                flat = self.sc.d2h(d_masks, len(tiles) * self.N, np.uint8).reshape(len(tiles), self.N)
                out = {t: flat[i].copy() for i, t in enumerate(tiles)}
            else:
                out = {t: np.zeros(0, dtype=np.uint8) for t in tiles}
            return lane_row, tile_rows, out
        finally:
            if d_masks:
                self.sc.free(d_masks)

    def consensus(self, max_d: int = 0, max_family: int = 256):
        """After finish(), any number of times, before or after every other pass (wd_lane_consensus,
        include/welldup_laneconsensus.h): the members of every family of 3 .. max_family wells under the labels the
        finish left are gathered, the code that more than half of them call at a cycle is the family's consensus there,
        and every member's calls are counted against it.
        -> (lane row int64 [20]: [Families, Wells, Profiled, Mismatches, WithN, Undecided, UndecidedCalls, FirstWellOff,
        PairFamilies, LargeFamilies, LargeWells, Dist d = 0..7 and >= 8], tile rows int64 [max_tiles, 4]: [Wells,
        Profiled, Mismatches, WithN] by the well's own tile, calls int64 [L, 5, 5]: [cycle][consensus][own code] over
        the wells with d <= max_d at the cycles their family decides).  The scratch is allocated for the call and
        released.  max_d outside 0..7, max_family outside 3..4096 or a call before a successful finish raises
        ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        lane_row = np.zeros(_lib.LANECONSENSUS_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANECONSENSUS_TILE_COLS), dtype=np.int64)
        calls = np.zeros((self.L, 5, 5), dtype=np.int64)
        self._with_scratch(self.sc.lane_consensus_scratch_bytes(self.max_tiles, self.N, self.L),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_consensus(
                               self._h, int(max_d), int(max_family), d_scratch, sbytes,
                               lane_row.ctypes.data_as(ctypes.c_void_p), tile_rows.ctypes.data_as(ctypes.c_void_p),
                               calls.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows, calls

    def hops(self, split: int, max_e: int, keys):
        """After finish() of a lane with an index part, any number of times, before or after index_finish and every
        other pass (wd_lane_hops, include/welldup_lanehops.h): the index key of every redundant well against its
        root's under the labels the finish left.  split: the cycles of the first index read, 1..I (I: a single
        index); max_e: the differing cycles an index read may have and still count as a read error, 0..3; keys: up
        to 1024 distinct index keys (uint64), the listed libraries.
        -> (lane row int64 [13]: [Pairs, SameTile, Hop1, Hop2, State[0..8]] with State[3 s1 + s2], s = 0 Same, 1 Near,
        2 Far, tile rows int64 [max_tiles, 4]: [Pairs, SameTile, Hop1, Hop2] by the copy's tile, matrix int64
        [M + 1, M + 1]: [root's rank][copy's rank], rank M = a key that is not listed).  The scratch is allocated for
        the call and released.  A bad split, max_e or list of keys, a lane without an index part, a tile that has
        reads but no index planes (or the reverse) or a call before a successful finish raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        listed = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1))
        M = int(listed.size)
        lane_row = np.zeros(_lib.LANEHOPS_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEHOPS_TILE_COLS), dtype=np.int64)
        matrix = np.zeros((min(M, _lib.LANEHOPS_MAX_LISTED) + 1,) * 2, dtype=np.int64)
        self._with_scratch(self.sc.lane_hops_scratch_bytes(self.max_tiles, M),      # (M > 1024 raises here)
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_hops(
                               self._h, int(split), int(max_e), M, listed.ctypes.data_as(ctypes.c_void_p) if M else None,
                               d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                               tile_rows.ctypes.data_as(ctypes.c_void_p), matrix.ctypes.data_as(ctypes.c_void_p)))
        return lane_row, tile_rows, matrix

    def distances(self, x, y, radius: int, matrix: bool = True):
        """After finish(), any number of times, before or after index_finish and mismatches (wd_lane_distances,
        include/welldup_lanedistance.h): every redundant well against its root under the labels the finish left, by
        where the two lie.  x, y: the coordinates of a tile's N wells, each 0 .. 2^24 - 1.
        -> (lane row int64 [14]: [Pairs, SameTile, Local, Dist[0..10]], tile rows int64 [max_tiles, 3]: [Pairs,
        SameTile, Local] by the member's tile, tile pairs int64 [max_tiles, max_tiles]: [root's tile][member's tile],
        or None without `matrix`).  The scratch is allocated for the call and released.  A radius outside 0 .. 2^25,
        a coordinate out of range or a call before a successful finish raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        xs, ys = self._coords(x, y)
        lane_row = np.zeros(_lib.LANEDISTANCE_LANE_COLS, dtype=np.int64)
        tile_rows = np.zeros((self.max_tiles, _lib.LANEDISTANCE_TILE_COLS), dtype=np.int64)
        tile_pairs = np.zeros((self.max_tiles, self.max_tiles), dtype=np.int64) if matrix else None
        self._with_scratch(self.sc.lane_distance_scratch_bytes(self.N, self.max_tiles, matrix),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_distances(
                               self._h, xs.ctypes.data_as(ctypes.c_void_p), ys.ctypes.data_as(ctypes.c_void_p), int(radius),
                               d_scratch, sbytes, lane_row.ctypes.data_as(ctypes.c_void_p),
                               tile_rows.ctypes.data_as(ctypes.c_void_p),
                               tile_pairs.ctypes.data_as(ctypes.c_void_p) if matrix else None))
        return lane_row, tile_rows, tile_pairs

    def saturation(self, steps: int, seed: int = 0, x=None, y=None, radius: int = 0):
        """After finish(), any number of times, before or after every other pass that follows a finish
        (wd_lane_saturation, include/welldup_lanesaturation.h): the lane's saturation curve under the labels the
        finish left.  Every PF well gets a step 0 .. steps - 1 from a hash of its global id and `seed` (uint32); with
        x, y (the coordinates of a tile's N wells, each 0 .. 2^24 - 1) and radius > 0 the same-tile copies closer
        than radius to their root - `distances`' Local - are dropped.
        -> (head int64 [2]: [PF, Dropped], new reads int64 [steps]: the counted wells of each step, new distinct
        int64 [steps]: the distinct reads that first appear in each step).  The scratch is allocated for the call
        and released.  steps outside 1..64, a seed outside uint32, a radius outside 0 .. 2^25 or without
        coordinates, one of x and y alone, a coordinate out of range or a call before a successful finish raises
        ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        if not 0 <= int(seed) < 1 << 32:
            raise ValueError("the seed is a uint32, not %d" % seed)
        if (x is None) != (y is None):
            raise ValueError("x and y come together or not at all")
        coords = x is not None
        xs = ys = None
        if coords:
            xs, ys = self._coords(x, y)
        n = min(max(int(steps), 1), _lib.LANESATURATION_MAX_STEPS)     # (the library refuses steps out of range)
        head = np.zeros(_lib.LANESATURATION_HEAD_COLS, dtype=np.int64)
        new_reads = np.zeros(n, dtype=np.int64)
        new_distinct = np.zeros(n, dtype=np.int64)
        self._with_scratch(self.sc.lane_saturation_scratch_bytes(self.N, self.max_tiles, coords),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_saturation(
                               self._h, int(steps), int(seed), xs.ctypes.data_as(ctypes.c_void_p) if coords else None,
                               ys.ctypes.data_as(ctypes.c_void_p) if coords else None, int(radius), d_scratch, sbytes,
                               head.ctypes.data_as(ctypes.c_void_p), new_reads.ctypes.data_as(ctypes.c_void_p),
                               new_distinct.ctypes.data_as(ctypes.c_void_p)))
        return head, new_reads, new_distinct

    def top(self, n_top: int, cand_capacity: int = 0):
        """After finish(), any number of times, before or after every other pass that follows a finish (wd_lane_top,
        include/welldup_lanetop.h): the lane's duplication levels and its n_top largest groups under the labels the
        finish left - classes, or clusters after a near finish -, ordered by size descending, then root ascending.
        -> (head int64 [4]: [PF, Groups2, Listed, Covered], levels int64 [2, 16]: Groups and Wells per level, root
        uint32 [n], size uint32 [n], exact uint32 [n]: the group's wells whose read equals the root's, tile_count uint32
        [n, max_tiles], reads: list of n str, the roots' reads), cut to n = Listed.  cand_capacity: how many candidate
        roots the selection may gather (0: 65536, raised to n_top); the result does not depend on it.  The scratch is
        allocated for the call and released.  n_top outside 1..1024, a capacity that is negative or positive and
        below n_top, or a call before a successful finish raises ValueError."""
        if self._h is None:
            raise ValueError("the accumulator is closed")
        n = min(max(int(n_top), 1), _lib.LANETOP_MAX)                  # (the library refuses what is out of range)
        cap = int(cand_capacity)
        head = np.zeros(_lib.LANETOP_HEAD_COLS, dtype=np.int64)
        levels = np.zeros((2, _lib.LANETOP_LEVELS), dtype=np.int64)
        root, size, exact = (np.zeros(n, dtype=np.uint32) for _ in range(3))
        tile_count = np.zeros((n, self.max_tiles), dtype=np.uint32)
        reads = np.zeros((n, self.L), dtype=np.uint8)
        ok = 1 <= int(n_top) <= _lib.LANETOP_MAX and (cap == 0 or n <= cap < 1 << 32)
        self._with_scratch(self.sc.lane_top_scratch_bytes(self.N, self.max_tiles, self.L, n, cap if ok else 0),
                           lambda d_scratch, sbytes: self.sc._lib.wd_lane_top(
                               self._h, int(n_top), cap, d_scratch, sbytes, head.ctypes.data_as(ctypes.c_void_p),
                               levels.ctypes.data_as(ctypes.c_void_p), root.ctypes.data_as(ctypes.c_void_p),
                               size.ctypes.data_as(ctypes.c_void_p), exact.ctypes.data_as(ctypes.c_void_p),
                               tile_count.ctypes.data_as(ctypes.c_void_p), reads.ctypes.data_as(ctypes.c_void_p)))
        k = int(head[2])
        return (head, levels, root[:k], size[:k], exact[:k], tile_count[:k],
                [reads[i].tobytes().decode("ascii") for i in range(k)])

    def _end(self):
        if self._h is not None:
            self.sc._lib.wd_lane_dups_end(self._h)
            self._h = None

    def close(self):
        """Drops the lane, finished or not, and frees the workspace."""
        self._end()
        for attr in ["d_ws", "d_labels", "d_near_labels", "d_mol"] + ["d_" + name for name in _SIDE_PARTS]:
            self.sc.free(getattr(self, attr))
            setattr(self, attr, 0)


class TileBatch:
    """BCL planes + filter bytes of a list of tiles, resident in HBM.

    Layout: planes[tile][cycle][N_pad] and filters[tile][N_pad], N_pad = N rounded up to
    256 bytes - or, with interleave=4, planes[tile][cycle // 4][N_pad][4]: the four cycles of a
    group side by side per well (include/welldup.h, wd_interleave4), which the equality /
    Hamming scan of sampled targets reads in half the cache lines.  Fill with `fill_synthetic`
    (device generator) or `upload_tile` (host bytes).
    """

    def __init__(self, scanner: Scanner, n_tiles: int, L: int, n_clusters: int, interleave: int = 1,
                 reuse: Optional["TileBatch"] = None):
        """reuse: a batch that is done with - its buffers are taken over when they are large enough
        (freeing device memory waits for every kernel in flight), else freed."""
        assert interleave in (1, 4)
        self.sc = scanner
        self.n_tiles, self.L, self.N = n_tiles, L, n_clusters
        self.interleave = interleave
        self.n_pad = (n_clusters + PLANE_ALIGN - 1) // PLANE_ALIGN * PLANE_ALIGN
        self.groups = (L + interleave - 1) // interleave          # plane slots per tile
        self.slot_bytes = self.n_pad * interleave
        self.plane_bytes = n_tiles * self.groups * self.slot_bytes
        self.filter_bytes = n_tiles * self.n_pad
        tmp_bytes = 4 * self.n_pad if interleave == 4 else 0
        if (reuse is not None and reuse.sc is scanner and reuse.d_planes and reuse._cap[0] >= self.plane_bytes
                and reuse._cap[1] >= self.filter_bytes and reuse._cap[2] >= tmp_bytes):
            self.d_planes, self.d_filters, self.d_tmp, self._cap = reuse.d_planes, reuse.d_filters, reuse.d_tmp, reuse._cap
            reuse.d_planes = reuse.d_filters = reuse.d_tmp = 0
        else:
            if reuse is not None:
                reuse.free()
            self.d_planes = scanner.malloc(max(1, self.plane_bytes))
            self.d_filters = scanner.malloc(max(1, self.filter_bytes))
            self.d_tmp = scanner.malloc(tmp_bytes) if tmp_bytes else 0
            self._cap = (self.plane_bytes, self.filter_bytes, tmp_bytes)
        self.tables = Scanner._tables(self.plane_ptrs(), self.filter_ptrs(), L)
        # dup_sets, tile_dups, tile_near_dups: a workspace each (a caller may interleave the calls) with the labels
        # behind it, allocated on first use, kept with the buffers: name -> [device address, capacity in bytes]
        self._ws = {name: [0, 0] for name in ("sets", "tdups", "tnear")}
        self.sets_bytes, self.edges = 0, 0
        if reuse is not None and reuse.sc is scanner:
            self.sets_bytes = reuse.sets_bytes if reuse.d_sets else 0
            self._ws, reuse._ws = reuse._ws, self._ws

    d_sets = property(lambda self: self._ws["sets"][0])
    d_tdups = property(lambda self: self._ws["tdups"][0])
    d_tnear = property(lambda self: self._ws["tnear"][0])

    def plane_ptr(self, tile: int, cycle: int) -> int:
        """Address of well 0 of the cycle (wells are `interleave` bytes apart)."""
        g, sub = divmod(cycle, self.interleave)
        return self.d_planes + (tile * self.groups + g) * self.slot_bytes + sub

    def _put_plane(self, tile: int, cycle: int, produce):
        """produce(dst) writes one plain N-byte plane at dst; lands it in this batch's layout."""
        if self.interleave == 1:
            produce(self.plane_ptr(tile, cycle))
            return
        sub = cycle % 4
        produce(self.d_tmp + sub * self.n_pad)
        if sub == 3 or cycle == self.L - 1:                       # the group is complete
            src = (ctypes.c_void_p * 4)(*[self.d_tmp + i * self.n_pad if i <= sub else None for i in range(4)])
            self.sc._ck(self.sc._lib.wd_interleave4(self.sc._ctx, src, self.N,
                                                    ctypes.c_void_p(self.plane_ptr(tile, cycle - sub))))
            self.sc.synchronize()                                 # d_tmp is reused by the next group

    def filter_ptr(self, tile: int) -> int:
        return self.d_filters + tile * self.n_pad

    def plane_ptrs(self) -> List[List[int]]:
        return [[self.plane_ptr(i, c) for c in range(self.L)] for i in range(self.n_tiles)]

    def filter_ptrs(self) -> List[int]:
        return [self.filter_ptr(i) for i in range(self.n_tiles)]

    def fill_synthetic(self, spec, lane_tile: Sequence, cycles: Sequence[int]):
        """lane_tile: [(lane, tile number)] per batch slot; cycles: the L 0-based cycles."""
        assert len(lane_tile) == self.n_tiles and len(cycles) == self.L
        assert spec.n_clusters == self.N
        for i, (lane, tile) in enumerate(lane_tile):
            self.sc.synth_filter(self.filter_ptr(i), spec, lane, tile)
            for c, cyc in enumerate(cycles):
                self._put_plane(i, c, lambda dst, cyc=cyc: self.sc.synth_plane(dst, spec, lane, tile, cyc))
        self.sc.synchronize()

    def upload_tile(self, slot: int, planes: Iterable[np.ndarray], filt: np.ndarray):
        for c, p in enumerate(planes):
            assert p.shape[0] == self.N
            self._put_plane(slot, c, lambda dst, p=p: self.sc.h2d(dst, np.ascontiguousarray(p, dtype=np.uint8)))
        assert filt.shape[0] == self.N
        self.sc.h2d(self.filter_ptr(slot), np.ascontiguousarray(filt, dtype=np.uint8))

    def download_plane(self, slot: int, cycle: int) -> np.ndarray:
        if self.interleave == 1:
            return self.sc.d2h(self.plane_ptr(slot, cycle), self.N)
        g, sub = divmod(cycle, 4)
        group = self.sc.d2h(self.plane_ptr(slot, 4 * g), 4 * self.N)
        return np.ascontiguousarray(group[sub::4])

    def download_filter(self, slot: int) -> np.ndarray:
        return self.sc.d2h(self.filter_ptr(slot), self.N)

    def count(self, mode: int, k: int, per_target: bool = False):
        self.sc.set_option("well_stride", self.interleave)
        try:
            return self.sc.count_tiles(None, self.filter_ptrs(), self.N, mode, k, per_target,
                                       tables=self.tables, L=self.L)
        finally:
            self.sc.set_option("well_stride", 1)

    def _with_workspace(self, name: str, ws: int, labels: bool, call):
        """Grows the workspace `name` to ws bytes plus the labels behind it and runs call(workspace address, label
        addresses or None) under this batch's well_stride.  -> (its result, labels uint32 [n_tiles, N] or None)."""
        w = self._ws[name]
        lbl_bytes = 4 * self.N * self.n_tiles if labels else 0
        if not w[0] or w[1] < ws + lbl_bytes:
            if w[0]:
                self.sc.free(w[0])
                w[0] = 0
            w[1] = ws + lbl_bytes
            w[0] = self.sc.malloc(max(1, w[1]))
        d_lbl = w[0] + ws
        lbl_ptrs = [d_lbl + 4 * self.N * i for i in range(self.n_tiles)] if labels else None
        self.sc.set_option("well_stride", self.interleave)
        try:
            out = call(w[0], lbl_ptrs)
        finally:
            self.sc.set_option("well_stride", 1)
        return out, (self.sc.d2h(d_lbl, lbl_bytes, np.uint32).reshape(self.n_tiles, self.N) if labels else None)

    def dup_sets(self, mode: int, k: int, labels: bool = False, edge_cap: int = 0):
        """count() plus the duplicate sets of every tile (Scanner.dup_sets; every well must be a target).
        -> (blocks, sets rows, labels uint32 [n_tiles, N] or None).  edges_processed is left in self.edges."""
        ws = self.sets_bytes = self.sc.dup_sets_workspace_bytes(self.N, self.n_tiles)
        (blocks, sets, self.edges), lab = self._with_workspace("sets", ws, labels, lambda d_ws, lbl_ptrs: self.sc.dup_sets(
            None, self.filter_ptrs(), self.N, mode, k, d_ws, ws, labels=lbl_ptrs, edge_cap=edge_cap, tables=self.tables,
            L=self.L))
        return blocks, sets, lab

    def tile_dups(self, labels: bool = False, hash_bits: int = 0):
        """The read classes of every tile of the batch (Scanner.tile_dups; every well must be a target, the
        batch a plane per cycle).  -> (rows, labels uint32 [n_tiles, N] or None)."""
        ws = self.sc.tile_dups_workspace_bytes(self.N, self.n_tiles)
        return self._with_workspace("tdups", ws, labels, lambda d_ws, lbl_ptrs: self.sc.tile_dups(
            None, self.filter_ptrs(), self.N, d_ws, ws, labels=lbl_ptrs, hash_bits=hash_bits, tables=self.tables, L=self.L))

    def tile_near_dups(self, k: int, labels: bool = False, pair_budget: int = 0, hash_bits: int = 0):
        """The near-duplicate clusters (Hamming distance <= k) of every tile of the batch (Scanner.tile_near_dups;
        every well must be a target, the batch a plane per cycle).  -> (rows, labels uint32 [n_tiles, N] or None)."""
        ws = self.sc.tile_near_dups_workspace_bytes(self.N, self.n_tiles, k)
        return self._with_workspace("tnear", ws, labels, lambda d_ws, lbl_ptrs: self.sc.tile_near_dups(
            None, self.filter_ptrs(), self.N, k, d_ws, ws, labels=lbl_ptrs, hash_bits=hash_bits, pair_budget=pair_budget,
            tables=self.tables, L=self.L))

    def free(self):
        for ptr in [self.d_planes, self.d_filters, self.d_tmp] + [w[0] for w in self._ws.values()]:
            if ptr:
                self.sc.free(ptr)
        self.d_planes = self.d_filters = self.d_tmp = 0
        for w in self._ws.values():
            w[0] = 0
