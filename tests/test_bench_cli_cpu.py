"""bench.py's command line: a plain run times the headline and nothing else; what takes runs of its own (sub-legs, RCCL leg,
box calibration, CPU baseline) runs only with --full."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_the_headline_alone():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert not a.full
    assert (a.gpus, a.steps, a.warmup, a.mode, a.batch, a.dump_outputs) == (1, 7, 3, "train", 64, None)
    d = bench.parse_args([])
    assert (d.steps, d.warmup) == (10, 2)


def test_full_brings_the_sub_legs_back():
    a = bench.parse_args(["--full"])
    assert a.full and not a.no_extras and not a.no_cpu_baseline
    a = bench.parse_args(["--full", "--no-extras", "--no-cpu-baseline", "--mode", "longform"])
    assert a.full and a.no_extras and a.no_cpu_baseline and a.batch == 256
