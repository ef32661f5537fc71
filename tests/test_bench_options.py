"""bench.py's plain run makes only the headline measurement; `--full` adds the side measurements (exact-fp32 steps,
strong-scaling ceiling, CPU baseline) that the configuration supports, and the --no-* switches still turn single ones off."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

NONE = {"fp32": False, "ceiling": False, "cpu_baseline": False}
ALL = {"fp32": True, "ceiling": True, "cpu_baseline": True}


def _args(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + list(argv))
    return bench.parse()


@pytest.mark.parametrize("argv", [(), ("--gpus", "1", "--steps", "20", "--warmup", "5"), ("--config", "listener"),
                                  ("--dump-outputs", "out"), ("--exact",)])
def test_plain_run_has_no_side_measurements(monkeypatch, argv):
    args = _args(monkeypatch, *argv)
    assert args.full is False
    assert bench.side_measurements(args, dist_on=False) == NONE


def test_full_run_has_every_side_measurement(monkeypatch):
    assert bench.side_measurements(_args(monkeypatch, "--full"), dist_on=False) == ALL
    assert bench.side_measurements(_args(monkeypatch, "--full", "--config", "listener"), dist_on=False) == ALL


def test_full_run_follows_the_configuration(monkeypatch):
    # (one rank only; no ceiling for the detector / joint configs, strong scaling, the small scenes or at fp32)
    assert bench.side_measurements(_args(monkeypatch, "--full"), dist_on=True) == NONE
    for argv in (("--config", "detector"), ("--config", "joint"), ("--scaling", "strong"), ("--small",)):
        assert bench.side_measurements(_args(monkeypatch, "--full", *argv), dist_on=False) == dict(ALL, ceiling=False), argv
    assert bench.side_measurements(_args(monkeypatch, "--full", "--exact"), dist_on=False) == dict(NONE, cpu_baseline=True)


def test_no_switches_turn_single_measurements_off(monkeypatch):
    for flag, key in (("--no-fp32", "fp32"), ("--no-ceiling", "ceiling"), ("--no-cpu-baseline", "cpu_baseline")):
        assert bench.side_measurements(_args(monkeypatch, "--full", flag), dist_on=False) == dict(ALL, **{key: False}), flag
        assert bench.side_measurements(_args(monkeypatch, flag), dist_on=False) == NONE, flag
