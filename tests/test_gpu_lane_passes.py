"""The passes after a lane's finish, driven from one table (well_duplicates_amd/lane_passes.py), through the CLI: every
pass in one run over two lanes, and the batches of the side cycles on an error."""
import io
import os
import re
import shutil
from contextlib import redirect_stdout

import pytest

from test_lane_passes_host import ORDER
from well_duplicates_amd import count_well_duplicates as cwd
from well_duplicates_amd import synth

pytestmark = pytest.mark.gpu

ROWS, COLS, LEVELS, L, SCAN = 36, 70, 3, 24, 15
NAMES = ["1101", "1102", "1103", "1104"]
# the first letters of a pass's tags, in the order the blocks print
TAGS = ["LaneMismatch", "LaneDistance", "LaneQualit", "LaneSaturation", "LaneTop", "LaneHop", "LaneGC", "LaneConsensus", "LaneUmi",
        "LaneKeep"]
INDEX = ["--lane-dups-index", "%d-%d,%d-%d" % (SCAN, SCAN + 3, SCAN + 3, SCAN + 6)]
UMI = ["--lane-dups-umi", "%d-%d" % (SCAN + 6, L), "--lane-dups-umi-mismatches", "0"]
# every pass with its max-d / radius given, so that no block depends on another pass's default
PASS_ARGV = {
    "LaneMismatch": ["--lane-dups-mismatches", "--lane-dups-mismatches-max-d", "2"],
    "LaneDistance": ["--lane-dups-distance", "--lane-dups-distance-radius", "2500"],
    "LaneQualit": ["--lane-dups-quality", "--lane-dups-quality-max-d", "2"],
    "LaneSaturation": ["--lane-dups-saturation", "--lane-dups-saturation-radius", "2500"],
    "LaneTop": ["--lane-dups-top", "5"],
    "LaneHop": ["--lane-dups-hops"],
    "LaneGC": ["--lane-dups-gc"],
    "LaneConsensus": ["--lane-dups-consensus", "--lane-dups-consensus-max-d", "2"],
    "LaneUmi": UMI,
    "LaneKeep": ["--lane-dups-keep", "--lane-dups-keep-umi"],
}
REQUIRES = {"LaneHop": INDEX, "LaneKeep": UMI}


def build_run_dir(run):
    """The run directory of test_gpu_lanemolecules.py's CLI test - 36 x 70 wells, four tiles, 24 cycles, tile 1103's files
    tile 1101's but for the last cycle, which is tile 1102's - with a second lane that holds the same files."""
    n = ROWS * COLS
    x, y = synth.honeycomb_pixels(ROWS, COLS)
    spec = synth.SynthSpec(seed=35, n_clusters=n, row=COLS, plant_per_64k=8000, nocall_per_64k=500, plant_far=True)
    synth.write_run_dir(spec, run, [1], NAMES, list(range(L)), slocs=synth.slocs_bytes(x, y))
    calls = os.path.join(run, "Data", "Intensities", "BaseCalls")
    ldir = os.path.join(calls, "L001")
    shutil.copy(os.path.join(ldir, "s_1_1101.filter"), os.path.join(ldir, "s_1_1103.filter"))
    for c in range(L):
        cdir = os.path.join(ldir, "C%d.1" % (c + 1))
        shutil.copy(os.path.join(cdir, "s_1_%s.bcl.gz" % ("1101" if c < L - 1 else "1102")), os.path.join(cdir, "s_1_1103.bcl.gz"))
    for root, _, files in os.walk(ldir):
        other = root.replace(ldir, os.path.join(calls, "L002"))
        os.makedirs(other, exist_ok=True)
        for f in files:
            shutil.copy(os.path.join(root, f), os.path.join(other, f.replace("s_1_", "s_2_")))
    return run


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    return build_run_dir(str(tmp_path_factory.mktemp("lane_passes") / "run"))


def _argv(run, lanes, extra):
    return ["-s", "hiseq_x", "-r", run, "-t", ",".join(NAMES), "-i", lanes, "-l", str(LEVELS), "--cycles", "0-%d" % SCAN, "-q",
            "--all-wells", "--lane-dups", "--lane-dups-hamming", "2"] + extra


def _main(argv):
    out = io.StringIO()
    with redirect_stdout(out):
        assert cwd.main(argv) == 0
    return out.getvalue()


def _blocks(text, lane):
    """stdout -> ([the passes' tags in the order their blocks start], {tag: the block's text}) for one lane."""
    order, blocks = [], {}
    for line in text.splitlines(keepends=True):
        m = re.match(r"(\w+): (\d+)\b", line)
        tag = next((t for t in TAGS if m and m.group(1).startswith(t)), None)
        if tag is None or m.group(2) != lane:
            continue
        if not order or order[-1] != tag:
            order.append(tag)
        blocks[tag] = blocks.get(tag, "") + line
    return order, blocks


def test_every_pass_at_once_prints_the_blocks_of_the_passes_alone(run_dir, tmp_path):
    """Two lanes, --tile-batch 3, --lane-dups-hamming 2 and all ten passes: the blocks appear once per lane in the
    documented order, each is byte for byte its block from a run with that pass alone (plus what it requires:
    --lane-dups-index for the hops, --lane-dups-umi for the keep per molecule), and lane 2, which holds lane 1's files
    and restarts lane 1's accumulator with its quality, index and UMI parts on, prints lane 1's blocks."""
    assert [PASS_ARGV[t][0] for t in TAGS] == ORDER
    everything = INDEX + [a for t in TAGS for a in PASS_ARGV[t]]
    out = _main(_argv(run_dir, "1,2", everything + ["--tile-batch", "3"]))
    per_lane = {lane: _blocks(out, lane) for lane in ("1", "2")}
    for lane in ("1", "2"):
        assert per_lane[lane][0] == TAGS, lane                          # once each, in the documented order
    assert out.index("LaneKeepSummary: 1\t") < out.index("LaneDupsSummary: 2\t")
    renumbered = {t: re.sub(r"(?m)^(\w+): 2\b", r"\1: 1", b) for t, b in per_lane["2"][1].items()}
    assert renumbered == per_lane["1"][1]
    assert all(per_lane["1"][1][t].count("\n") >= 1 for t in TAGS)
    for tag in TAGS:
        alone = _main(_argv(run_dir, "1", REQUIRES.get(tag, []) + PASS_ARGV[tag]))
        order, blocks = _blocks(alone, "1")
        assert order == ([t for t in TAGS if t in (tag, "LaneUmi")] if tag == "LaneKeep" else [tag]), tag
        assert blocks[tag] == per_lane["1"][1][tag], tag


def test_the_side_batches_are_freed_when_a_later_lane_fails(run_dir, monkeypatch):
    """Lane 1 in four batches with --lane-dups-umi, then a lane whose directory is missing: the batches of UMI cycles
    that the finished scan batches left to be taken over are freed with them when the error leaves scan_lanes, after
    lane 1 has been reported."""
    made = []

    class Recording(cwd.TileBatch):
        def __init__(self, *args, **kwargs):
            super().__init__(*args, **kwargs)
            made.append(self)

    monkeypatch.setattr(cwd, "TileBatch", Recording)
    out = io.StringIO()
    with redirect_stdout(out), pytest.raises(FileNotFoundError):
        cwd.main(_argv(run_dir, "1,3", UMI + ["--tile-batch", "1"]))
    assert "LaneDupsSummary: 1\t" in out.getvalue() and "LaneUmiSummary: 1\t" in out.getvalue()
    assert not re.search(r"(?m)^Lane\w*: 3\t", out.getvalue())             # nothing of the lane that is not there
    assert len(made) >= 8 and {tb.L for tb in made} == {SCAN, L - SCAN - 6}
    assert [tb.L for tb in made if tb.d_planes] == []                  # freed, or taken over by a later batch
