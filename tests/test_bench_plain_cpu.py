"""bench.py's plain run against `--full` without a GPU: a plain run asks for none of the legs beside the headline,
`--full` asks for them as before, and the opt-out flags still hold under `--full`."""
import pytest


@pytest.mark.parametrize("argv", [[], ["--steps", "10", "--warmup", "2"], ["--workload", "spectrum16k"],
                                  ["--gpus", "2", "--dry-run"]])
def test_plain_run_asks_for_nothing_beside_the_headline(argv):
    import bench
    args = bench.parse_args(argv)
    assert not args.full
    assert args.no_cpu_baseline and args.no_also and not args.measure_traffic and not args.gather


def test_full_asks_for_the_legs():
    import bench
    args = bench.parse_args(["--full"])
    assert args.full and not args.no_cpu_baseline and not args.no_also


def test_opt_outs_hold_under_full():
    import bench
    args = bench.parse_args(["--full", "--no-also", "--no-cpu-baseline", "--no-measure-traffic"])
    assert args.no_also and args.no_cpu_baseline and not args.measure_traffic


def test_gather_alone_does_not_bring_the_other_legs():
    import bench
    args = bench.parse_args(["--gpus", "2", "--gather"])
    assert args.gather and not args.full and args.no_also and args.no_cpu_baseline and not args.measure_traffic
