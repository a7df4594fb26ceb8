"""The passes that run after a lane's finish, as one table: the Python counterpart of csrc/lane_pass.inc (DESIGN 5.20,
5.20.1).

Every --lane-dups-<pass> of count_well_duplicates is one LanePass entry of ALL_PASSES, in the order the passes run
and print: LANE_PASSES, the ten passes up to --lane-dups-keep-umi in the order they were added, and the adapter pass,
which runs and prints after the GC pass.  The CLI's option checks, its defaults, the device memory check, the calls after a lane's finish, the lane's
blocks and the --...-out files all loop over this table; a pass is written down nowhere else in the driver.  The label
stage - finish, the near finish, the members and the index finish - is not a pass: it stays code in scan_lanes.
"""
from __future__ import annotations

import os
import struct
from collections import namedtuple

import numpy as np

from . import _lib, report, workload

# One option of a pass.  needs: the options it is refused without (a tuple inside: any one of them will do, the
# message names the first); lo, hi: the range it takes (hi None: no upper end); takes: what the message says it takes
# where that is not "lo..hi".
Option = namedtuple("Option", "flag needs lo hi takes", defaults=((), None, None, None))

# One pass.
#   key      where its counts go, results[key][lane]
#   flag     its name in the messages
#   options  its Options, for check_options
#   resolve  (args, run) -> its parameters, a dict, or None when the pass is not asked for; the defaults live here.
#            run: .xy (the coordinates of a tile's wells), .cycle_list, and for `bytes` .n_wells, .n_tiles
#   fit      the (keyword, flag) pairs of check_lane_dups_fits it owns, in the order of the message's clauses
#   bytes    (sc, run, params) -> {keyword: device bytes} (a keyword of another pass where the two share a region)
#   run      (ld, lane context, params) -> its Counts object.  The lane context: .names, .n_clusters, .cycle_list,
#            .lane_near, .left (the counts the lane was left with: the clusters' under lane_near, else the classes'),
#            .listing, .final, .index_lengths (of the index finish, or None), .reader, .lane
#   write    report.write_* (lane, counts, verbose=, out=)
#   out      (its --...-out option, report.write_*_tsv) or None
#   parts    params -> the per-batch parts of the accumulator it needs: "quality": the bin edges of the qualities kept
#            beside the reads; "sides": {name: cycles}, a further TileBatch of these cycles per scan batch, begun and
#            fed through LaneDups.<name>_begin / <name>_add
#   check    (args, error) for what the two shapes of `options` do not cover, or None
LanePass = namedtuple("LanePass", "key flag options resolve fit bytes run write out parts check",
                      defaults=(None, lambda params: {}, None))

DEFAULT_QUALITY_BINS = [0, 2, 10, 20, 25, 30, 35, 40]


def dest(flag):
    """--lane-dups-gc-bins -> lane_dups_gc_bins"""
    return flag[2:].replace("-", "_")


def given(args, flag):
    """Is the option on the command line?  (`--lane-dups-hops 0` is.)"""
    value = getattr(args, dest(flag))
    return value is not None and value is not False


def parse_quality_bins(text):
    """--lane-dups-quality-bins E0,E1,.. -> the edges (None: the default); ValueError says what is wrong with them."""
    if text is None:
        return list(DEFAULT_QUALITY_BINS)
    try:
        edges = [int(e) for e in text.split(",")]
    except ValueError:
        raise ValueError("a comma-separated list of integers, not %r" % text)
    if not 1 <= len(edges) <= _lib.LANEQUALITY_MAX_BINS:
        raise ValueError("1..%d lower edges, not %d" % (_lib.LANEQUALITY_MAX_BINS, len(edges)))
    if edges[0] != 0:
        raise ValueError("the first edge is 0 (every quality has a bin), not %d" % edges[0])
    if any(b < a for a, b in zip(edges, edges[1:])):
        raise ValueError("the edges ascend")
    if edges[-1] >= _lib.LANEQUALITY_VALUES:
        raise ValueError("a quality is at most %d, not %d" % (_lib.LANEQUALITY_VALUES - 1, edges[-1]))
    return edges


def check_cycle_ranges(error, flag, text, example, most):
    """--lane-dups-index / --lane-dups-umi RANGES: ranges as --cycles takes them, 1..most cycles in all."""
    try:
        ranges = workload.parse_cycles(0, 0, text)
    except ValueError:
        ranges = [(0, 0)]
    if any(not 0 <= a < b for a, b in ranges):
        error("%s takes ranges of cycles as --cycles does, eg. %s" % (flag, example))
    n = sum(b - a for a, b in ranges)
    if not 1 <= n <= most:
        error("%s takes 1..%d cycles, not %d" % (flag, most, n))


def check_options(args, error):
    """Every `needs`, then every range, then what is neither; error = ArgumentParser.error."""
    options = [o for p in ALL_PASSES for o in p.options]
    for o in options:
        for need in o.needs if given(args, o.flag) else ():
            any_of = (need,) if isinstance(need, str) else need
            if not any(given(args, f) for f in any_of):
                error("%s needs %s" % (o.flag, any_of[0]))
    for o in options:
        value = getattr(args, dest(o.flag))
        if o.lo is not None and given(args, o.flag) and not (o.lo <= value and (o.hi is None or value <= o.hi)):
            error("%s takes %s, not %d" % (o.flag, o.takes or "%d..%d" % (o.lo, o.hi), value))
    for p in ALL_PASSES:
        if p.check is not None:
            p.check(args, error)


def resolve_passes(args, run):
    """The passes a command line asks for, with their parameters: [(LanePass, params)] in the table's order."""
    resolved = [(p, p.resolve(args, run)) for p in ALL_PASSES]
    return [(p, params) for p, params in resolved if params is not None]


def _first(*values):
    return next(v for v in values if v is not None)


def _near_k(args):
    return args.lane_dups_hamming or 0


def _mismatch_d(args):
    if not args.lane_dups_mismatches:
        return None
    return _first(args.lane_dups_mismatches_max_d, _near_k(args))


def _check_mismatch(args, error):
    if args.lane_dups_mismatches and args.lane_dups_hamming is None:
        error("--lane-dups-mismatches needs --lane-dups-hamming K with K >= 1 (under equality every copy is identical "
              "to the first well of its class: there is nothing to profile)")


def _run_mismatch(ld, lc, p):
    """D (with lane_near): LaneDups.mismatches(D) -> LaneMismatchCounts, its cycles numbered by cycle_list."""
    return report.LaneMismatchCounts.from_rows(*ld.mismatches(p["d"]), lc.names, lc.lane_near, p["d"], lc.cycle_list)


def _resolve_distance(args, run):
    if not args.lane_dups_distance:
        return None
    return {"x": run.xy[0], "y": run.xy[1], "radius": args.lane_dups_distance_radius}


def _run_distance(ld, lc, p):
    """(x, y, radius), x and y the coordinates of a tile's wells: LaneDups.distances(x, y, radius), with the tile
    pair matrix up to LANEDISTANCE_MATRIX_MAX_TILES tiles -> LaneDistanceCounts."""
    lx, ly = p["x"], p["y"]
    area = float(int(lx.max()) - int(lx.min())) * float(int(ly.max()) - int(ly.min())) if len(lx) else 0.0
    rows = ld.distances(lx, ly, p["radius"], matrix=len(lc.names) <= _lib.LANEDISTANCE_MATRIX_MAX_TILES)
    return report.LaneDistanceCounts.from_rows(*rows, lc.names, p["radius"], lc.left, area)


def _check_quality(args, error):
    try:
        args.lane_dups_quality_edges = parse_quality_bins(args.lane_dups_quality_bins)
    except ValueError as e:
        error("--lane-dups-quality-bins: %s" % e)


def _resolve_quality(args, run):
    if not args.lane_dups_quality:
        return None
    return {"edges": args.lane_dups_quality_edges,
            "d": _first(args.lane_dups_quality_max_d, _mismatch_d(args), _near_k(args))}


def _quality_bytes(sc, run, p):
    """The quality part of the accumulator and the pass's scratch: --lane-dups-keep counts both too, under this
    pass's keyword - the two share the part."""
    return {"quality": sc.lane_qual_workspace_bytes(run.n_wells, run.n_tiles, len(run.cycle_list)) +
            sc.lane_qual_scratch_bytes(run.n_tiles)}


def _run_quality(ld, lc, p):
    """(edges, D): the accumulator gets a quality part with these bins, every batch is fed to LaneDups.qual_add beside
    add, and LaneDups.qualities(D) -> LaneQualityCounts."""
    return report.LaneQualityCounts.from_rows(*ld.qualities(p["d"]), lc.names, lc.lane_near, p["d"], p["edges"])


def _resolve_saturation(args, run):
    if not args.lane_dups_saturation:
        return None
    radius = _first(args.lane_dups_saturation_radius, args.lane_dups_distance_radius if args.lane_dups_distance else 0)
    return {"steps": _first(args.lane_dups_saturation_steps, 20), "seed": args.lane_dups_saturation_seed or 0,
            "x": run.xy[0] if radius else None, "y": run.xy[1] if radius else None, "radius": radius}


def _run_saturation(ld, lc, p):
    """(steps, seed, x, y, radius), x and y the coordinates of a tile's wells or None with radius 0:
    LaneDups.saturation(steps, seed, x, y, radius) -> LaneSaturationCounts."""
    return report.LaneSaturationCounts.from_rows(*ld.saturation(p["steps"], p["seed"], p["x"], p["y"], p["radius"]),
                                                 p["seed"], p["radius"], lc.left, lc.lane_near)


def _resolve_top(args, run):
    return None if args.lane_dups_top is None else {"n": args.lane_dups_top}


def _run_top(ld, lc, p):
    """N > 0: LaneDups.top(N) -> LaneTopCounts."""
    return report.LaneTopCounts.from_rows(*ld.top(p["n"]), p["n"], lc.n_clusters, lc.names, lc.left, lc.lane_near)


def _resolve_hops(args, run):
    if args.lane_dups_hops is None:
        return None
    return {"e": _first(args.lane_dups_hops_mismatches, 1), "pairs": args.lane_dups_hops}


def _run_hops(ld, lc, p):
    """(E, pairs to list) (with the index cycles): LaneDups.hops(cycles of the first index range, E, the keys of the
    first LANEHOPS_MAX_LISTED groups the index finish listed) -> LaneHopCounts."""
    keys = lc.listing[3][:_lib.LANEHOPS_MAX_LISTED]
    pf = [int(v) for v in lc.listing[2][:len(keys), 0]]
    return report.LaneHopCounts.from_rows(*ld.hops(lc.index_lengths[0], p["e"], keys), keys,
                                          pf + [int(lc.final[0]) - sum(pf)], lc.index_lengths, lc.names, p["e"],
                                          lc.lane_near, p["pairs"])


def _resolve_gc(args, run):
    if not args.lane_dups_gc:
        return None
    max_n = args.lane_dups_gc_max_n or 0
    if max_n > len(run.cycle_list):
        raise ValueError("--lane-dups-gc-max-n takes 0..%d, the scanned cycles, not %d" % (len(run.cycle_list), max_n))
    return {"max_n": max_n, "bins": args.lane_dups_gc_bins or 20}


def _run_gc(ld, lc, p):
    """(max_n, bins): LaneDups.gc(max_n) -> LaneGCCounts."""
    return report.LaneGCCounts.from_rows(*ld.gc(p["max_n"]), lc.names, p["max_n"], p["bins"], lc.lane_near)


ADAPTER_NAMES = {"truseq": "AGATCGGAAGAGC", "nextera": "CTGTCTCTTATACACATCT", "smallrna": "TGGAATTCTCGG"}


def parse_adapter(text):
    """--lane-dups-adapter NAME|SEQ -> (what the block calls it, its codes 0..3); ValueError lists the names."""
    seq = ADAPTER_NAMES.get(text.lower(), text.upper())
    if not (_lib.LANEADAPTER_MIN_LEN <= len(seq) <= _lib.LANEADAPTER_MAX_LEN and set(seq) <= set("ACGT")):
        raise ValueError("%s, or %d..%d letters of ACGT, not %r" % (
            ", ".join("%s (%s)" % item for item in ADAPTER_NAMES.items()), _lib.LANEADAPTER_MIN_LEN,
            _lib.LANEADAPTER_MAX_LEN, text))
    return (text.lower() if text.lower() in ADAPTER_NAMES else seq), ["ACGT".index(ch) for ch in seq]


def _check_adapter(args, error):
    if args.lane_dups_adapter is None:
        return
    try:
        m = len(parse_adapter(args.lane_dups_adapter)[1])
    except ValueError as e:
        error("--lane-dups-adapter takes %s" % e)
    if args.lane_dups_adapter_min_overlap is not None and args.lane_dups_adapter_min_overlap > m:
        error("--lane-dups-adapter-min-overlap takes %d..%d, the adapter's length, not %d" % (
            _lib.LANEADAPTER_MIN_OVERLAP, m, args.lane_dups_adapter_min_overlap))


def _resolve_adapter(args, run):
    if args.lane_dups_adapter is None:
        return None
    name, codes = parse_adapter(args.lane_dups_adapter)
    cycles = list(run.cycle_list)
    if any(b != a + 1 for a, b in zip(cycles, cycles[1:])):
        raise ValueError("--lane-dups-adapter takes scanned cycles that are one ascending run of consecutive cycles (a "
                         "position in a read that skips cycles is not an insert length), not --cycles %s" % args.cycles)
    overlap = _first(args.lane_dups_adapter_min_overlap, min(8, len(codes)))
    if overlap > len(cycles):
        raise ValueError("--lane-dups-adapter-min-overlap takes %d..%d, the scanned cycles, not %d" % (
            _lib.LANEADAPTER_MIN_OVERLAP, len(cycles), overlap))
    return {"name": name, "codes": codes, "e": _first(args.lane_dups_adapter_mismatches, 1), "overlap": overlap,
            "bins": args.lane_dups_adapter_bins or 10, "dimer": _first(args.lane_dups_adapter_dimer, 10)}


def _run_adapter(ld, lc, p):
    """(name, codes, E, O, bins, dimer): LaneDups.adapter(codes, E, O) -> LaneAdapterCounts, its positions numbered
    from the first scanned cycle."""
    return report.LaneAdapterCounts.from_rows(*ld.adapter(p["codes"], p["e"], p["overlap"]), lc.names, p["name"],
                                              len(p["codes"]), p["e"], p["overlap"], p["bins"], p["dimer"], lc.lane_near,
                                              lc.cycle_list[0] if lc.cycle_list else 0)


def _resolve_consensus(args, run):
    if not args.lane_dups_consensus:
        return None
    return {"d": _first(args.lane_dups_consensus_max_d, _mismatch_d(args), _near_k(args)),
            "max_family": args.lane_dups_consensus_max_family or 256}


def _run_consensus(ld, lc, p):
    """(D, max family): LaneDups.consensus(D, max family) -> LaneConsensusCounts, its cycles numbered by cycle_list."""
    return report.LaneConsensusCounts.from_rows(*ld.consensus(p["d"], p["max_family"]), lc.names, lc.lane_near, p["d"],
                                                p["max_family"], lc.left.pf, lc.cycle_list)


def _check_umi(args, error):
    if args.lane_dups_umi is not None:
        check_cycle_ranges(error, "--lane-dups-umi", args.lane_dups_umi, "0-8 or 151-160", _lib.LANEUMI_MAX_CYCLES)


def _resolve_umi(args, run):
    if not args.lane_dups_umi:
        return None
    return {"cycles": [c for s, e in workload.parse_cycles(0, 0, args.lane_dups_umi) for c in range(s, e)],
            "e": _first(args.lane_dups_umi_mismatches, 1), "max_family": args.lane_dups_umi_max_family or 256,
            "molecules": args.lane_dups_keep_umi}


def _run_umi(ld, lc, p):
    """(UMI cycles, E, max family, molecules): every batch gets a further TileBatch of the UMI cycles, loaded by the
    batch's job list and fed to LaneDups.umi_add, reused and released with the scan batch; LaneDups.umi(E, max
    family) -> LaneUmiCounts.  molecules (--lane-dups-keep-umi): the pass writes its molecules down for the keep."""
    return report.LaneUmiCounts.from_rows(*ld.umi(p["e"], p["max_family"], molecules=p["molecules"]), lc.names,
                                          lc.lane_near, p["e"], p["max_family"], len(p["cycles"]), lc.left.pf,
                                          lc.left.redundant)


def _resolve_keep(args, run):
    if not args.lane_dups_keep:
        return None
    return {"min_q": _first(args.lane_dups_keep_min_q, _lib.LANEKEEP_DEFAULT_MIN_Q),
            "edges": args.lane_dups_quality_edges, "out": args.lane_dups_keep_out,
            "by_molecule": args.lane_dups_keep_umi}


def _keep_bytes(sc, run, p):
    parts = dict(_quality_bytes(sc, run, p), keep=sc.lane_keep_scratch_bytes(run.n_tiles, run.n_wells))
    if p["by_molecule"]:
        parts["molecules"] = sc.lane_molecules_bytes(run.n_tiles, run.n_wells)
    return parts


def write_keep_filter(path, filter_bytes: np.ndarray, mask: np.ndarray):
    """A .filter file as bcl.Tile.read_filter reads it: the 12-byte header (0, 3, N), then N bytes, each the input
    file's byte with bit 0 replaced by the mask's - 1 for a kept well, 0 for any other."""
    filt, mask = np.asarray(filter_bytes, dtype=np.uint8), np.asarray(mask, dtype=np.uint8)
    if filt.shape != mask.shape or filt.ndim != 1:
        raise ValueError("a filter of %s bytes and a mask of %s" % (filt.shape, mask.shape))
    with open(path, "wb") as fh:
        fh.write(struct.pack("<III", 0, 3, filt.shape[0]))
        fh.write(((filt & 0xFE) | (mask & 1)).astype(np.uint8).tobytes())


def write_lane_keep_filters(out_dir, lane, tiles, masks):
    """--lane-dups-keep-out: out_dir/L00<lane>/<the name of the tile's own .filter file> for every tile of masks
    ({tile: uint8 [N]}, LaneDups.keep's by the tile's name); tiles = {tile: its bcl.Tile}.  -> the paths written."""
    lane_dir = str(lane) if str(lane).startswith("L") else "L%03d" % int(lane)
    os.makedirs(os.path.join(out_dir, lane_dir), exist_ok=True)
    paths = []
    for tile in sorted(masks, key=str):
        path = os.path.join(out_dir, lane_dir, os.path.basename(tiles[tile].filter_file))
        write_keep_filter(path, tiles[tile].read_filter(), masks[tile])
        paths.append(path)
    return paths


def _run_keep(ld, lc, p):
    """(min_q, edges, out directory or None, by molecule): the accumulator gets a quality part with these bins (the
    one --lane-dups-quality asks for: the two share it); LaneDups.keep(min_q) -> LaneKeepCounts.  by molecule needs
    the UMI pass before it, which then writes its molecules down (LaneDups.umi(molecules=True)) for the keep to read
    (by_molecule=True).  With a directory the lane's filter files go there at once; the masks, lane-sized, are not
    kept."""
    kept = ld.keep(p["min_q"], masks=p["out"] is not None, by_molecule=p["by_molecule"])
    counts = report.LaneKeepCounts.from_rows(kept[0], kept[1], lc.names, lc.lane_near, p["min_q"], p["edges"],
                                             len(lc.cycle_list), by="molecule" if p["by_molecule"] else None)
    if p["out"] is not None:
        write_lane_keep_filters(p["out"], lc.lane, {t: lc.reader.get_tile(lc.lane, t) for t in lc.names},
                                {lc.names[ti]: m for ti, m in kept[2].items()})
    return counts


LANE_PASSES = (
    LanePass("lmismatch", "--lane-dups-mismatches",
             (Option("--lane-dups-mismatches-max-d", ("--lane-dups-mismatches",), 0, _lib.LANEMISMATCH_MAX_D),),
             lambda args, run: None if _mismatch_d(args) is None else {"d": _mismatch_d(args)},
             (("mismatch", "--lane-dups-mismatches"),),
             lambda sc, run, p: {"mismatch": sc.lane_mismatch_scratch_bytes(run.n_tiles, len(run.cycle_list))},
             _run_mismatch, report.write_lane_mismatches, check=_check_mismatch),
    LanePass("ldistance", "--lane-dups-distance",
             (Option("--lane-dups-distance", ("--lane-dups",)),
              Option("--lane-dups-distance-radius", (), 0, _lib.LANEDISTANCE_MAX_RADIUS)),
             _resolve_distance, (("distance", "--lane-dups-distance"),),
             lambda sc, run, p: {"distance": sc.lane_distance_scratch_bytes(run.n_wells, run.n_tiles,
                                                                            run.n_tiles <= _lib.LANEDISTANCE_MATRIX_MAX_TILES)},
             _run_distance, report.write_lane_distances),
    LanePass("lquality", "--lane-dups-quality",
             (Option("--lane-dups-quality", ("--lane-dups",)),
              Option("--lane-dups-quality-bins", (("--lane-dups-quality", "--lane-dups-keep"),)),
              Option("--lane-dups-quality-max-d", ("--lane-dups-quality",), 0, _lib.LANEQUALITY_MAX_D)),
             _resolve_quality, (("quality", "--lane-dups-quality"),), _quality_bytes,
             _run_quality, report.write_lane_qualities, parts=lambda p: {"quality": p["edges"]}, check=_check_quality),
    LanePass("lsaturation", "--lane-dups-saturation",
             (Option("--lane-dups-saturation", ("--lane-dups",)),
              Option("--lane-dups-saturation-steps", ("--lane-dups-saturation",), 1, _lib.LANESATURATION_MAX_STEPS),
              Option("--lane-dups-saturation-seed", ("--lane-dups-saturation",), 0, (1 << 32) - 1),
              Option("--lane-dups-saturation-radius", ("--lane-dups-saturation",), 0, _lib.LANESATURATION_MAX_RADIUS)),
             _resolve_saturation, (("saturation", "--lane-dups-saturation"),),
             lambda sc, run, p: {"saturation": sc.lane_saturation_scratch_bytes(run.n_wells, run.n_tiles,
                                                                                p["radius"] > 0)},
             _run_saturation, report.write_lane_saturation),
    LanePass("ltop", "--lane-dups-top",
             (Option("--lane-dups-top", ("--lane-dups",), 1, _lib.LANETOP_MAX),
              Option("--lane-dups-top-out", ("--lane-dups-top",))),
             _resolve_top, (("top", "--lane-dups-top"),),
             lambda sc, run, p: {"top": sc.lane_top_scratch_bytes(run.n_wells, run.n_tiles, len(run.cycle_list), p["n"])},
             _run_top, report.write_lane_top, ("--lane-dups-top-out", report.write_lane_top_tsv)),
    LanePass("lhops", "--lane-dups-hops",
             (Option("--lane-dups-hops", ("--lane-dups-index",), 0, None, "the number of library pairs to list"),
              Option("--lane-dups-hops-mismatches", ("--lane-dups-hops",), 0, _lib.LANEHOPS_MAX_E),
              Option("--lane-dups-hops-out", ("--lane-dups-hops",))),
             _resolve_hops, (("hops", "--lane-dups-hops"),),
             lambda sc, run, p: {"hops": sc.lane_hops_scratch_bytes(run.n_tiles, _lib.LANEHOPS_MAX_LISTED)},
             _run_hops, report.write_lane_hops, ("--lane-dups-hops-out", report.write_lane_hops_tsv)),
    LanePass("lgc", "--lane-dups-gc",
             (Option("--lane-dups-gc", ("--lane-dups",)),
              Option("--lane-dups-gc-bins", ("--lane-dups-gc",), report.LANE_GC_MIN_BINS, report.LANE_GC_MAX_BINS),
              Option("--lane-dups-gc-max-n", ("--lane-dups-gc",), 0, None, "0..the number of scanned cycles"),
              Option("--lane-dups-gc-out", ("--lane-dups-gc",))),
             _resolve_gc, (("gc", "--lane-dups-gc"),),
             lambda sc, run, p: {"gc": sc.lane_gc_scratch_bytes(run.n_tiles, len(run.cycle_list))},
             _run_gc, report.write_lane_gc, ("--lane-dups-gc-out", report.write_lane_gc_tsv)),
    LanePass("lconsensus", "--lane-dups-consensus",
             (Option("--lane-dups-consensus", ("--lane-dups",)),
              Option("--lane-dups-consensus-max-d", ("--lane-dups-consensus",), 0, _lib.LANECONSENSUS_MAX_D),
              Option("--lane-dups-consensus-max-family", ("--lane-dups-consensus",), 3, _lib.LANECONSENSUS_MAX_FAMILY),
              Option("--lane-dups-consensus-out", ("--lane-dups-consensus",))),
             _resolve_consensus, (("consensus", "--lane-dups-consensus"),),
             lambda sc, run, p: {"consensus": sc.lane_consensus_scratch_bytes(run.n_tiles, run.n_wells,
                                                                              len(run.cycle_list))},
             _run_consensus, report.write_lane_consensus,
             ("--lane-dups-consensus-out", report.write_lane_consensus_tsv)),
    LanePass("lumi", "--lane-dups-umi",
             (Option("--lane-dups-umi", ("--lane-dups",)),
              Option("--lane-dups-umi-mismatches", ("--lane-dups-umi",), 0, _lib.LANEUMI_MAX_E),
              Option("--lane-dups-umi-max-family", ("--lane-dups-umi",), 2, _lib.LANEUMI_MAX_FAMILY),
              Option("--lane-dups-umi-out", ("--lane-dups-umi",))),
             _resolve_umi, (("umi", "--lane-dups-umi"), ("umi_scratch", "--lane-dups-umi")),
             lambda sc, run, p: {"umi": sc.lane_umi_workspace_bytes(run.n_wells, run.n_tiles, len(p["cycles"])),
                                 "umi_scratch": sc.lane_umi_scratch_bytes(run.n_tiles, run.n_wells)},
             _run_umi, report.write_lane_umi, ("--lane-dups-umi-out", report.write_lane_umi_tsv),
             parts=lambda p: {"sides": {"umi": p["cycles"]}}, check=_check_umi),
    LanePass("lkeep", "--lane-dups-keep",
             (Option("--lane-dups-keep", ("--lane-dups",)),
              Option("--lane-dups-keep-min-q", ("--lane-dups-keep",), 0, _lib.LANEKEEP_MAX_Q),
              Option("--lane-dups-keep-out", ("--lane-dups-keep",)),
              Option("--lane-dups-keep-umi", ("--lane-dups-keep", "--lane-dups-umi"))),
             _resolve_keep, (("keep", "--lane-dups-keep"), ("molecules", "--lane-dups-keep-umi")), _keep_bytes,
             _run_keep, report.write_lane_keep, parts=lambda p: {"quality": p["edges"]}),
)

# the eleventh pass: it runs and prints after the GC pass, whose loading of the rows and whose block it follows
ADAPTER_PASS = LanePass(
    "ladapter", "--lane-dups-adapter",
    (Option("--lane-dups-adapter", ("--lane-dups",)),
     Option("--lane-dups-adapter-mismatches", ("--lane-dups-adapter",), 0, _lib.LANEADAPTER_MAX_E),
     Option("--lane-dups-adapter-min-overlap", ("--lane-dups-adapter",), _lib.LANEADAPTER_MIN_OVERLAP, None,
            "%d..the adapter's length" % _lib.LANEADAPTER_MIN_OVERLAP),
     Option("--lane-dups-adapter-bins", ("--lane-dups-adapter",), report.LANE_ADAPTER_MIN_BINS, report.LANE_ADAPTER_MAX_BINS),
     Option("--lane-dups-adapter-dimer", ("--lane-dups-adapter",), 0, None, "an insert length of 0 or more"),
     Option("--lane-dups-adapter-out", ("--lane-dups-adapter",))),
    _resolve_adapter, (("adapter", "--lane-dups-adapter"),),
    lambda sc, run, p: {"adapter": sc.lane_adapter_scratch_bytes(run.n_tiles, len(run.cycle_list))},
    _run_adapter, report.write_lane_adapter, ("--lane-dups-adapter-out", report.write_lane_adapter_tsv),
    check=_check_adapter)
_AFTER = [p.key for p in LANE_PASSES].index("lgc") + 1
ALL_PASSES = LANE_PASSES[:_AFTER] + (ADAPTER_PASS,) + LANE_PASSES[_AFTER:]
