"""bench.py --full on the CPU: which measurements a run makes after its timed region (full_legs).  A plain run makes none; --full makes
every leg its --no-* switches leave on, the single-GPU legs at N = 1 only.  tests/test_gpu_fullsize.py runs both forms on the GPU."""


def _legs(argv, world=1):
    import bench
    return bench.full_legs(bench.parse_args(argv), world)


def test_a_plain_run_measures_nothing_after_its_timed_region():
    assert not any(_legs(["--gpus", "1", "--steps", "20", "--warmup", "5"]).values())
    assert not any(_legs(["--gpus", "2", "--steps", "20", "--warmup", "5"], world=2).values())


def test_full_runs_every_leg_at_one_gpu():
    assert all(_legs(["--steps", "20", "--warmup", "5", "--full"]).values())


def test_full_keeps_the_single_leg_switches():
    legs = _legs(["--full", "--no-cpu-baseline", "--val-dice-steps", "0"])
    assert legs == {"exclusive": True, "continuity": True, "val_dice": False, "secondary": True, "cpu_baseline": False}
    legs = _legs(["--full", "--no-secondary", "--no-exclusive-pass"])
    assert legs == {"exclusive": False, "continuity": False, "val_dice": True, "secondary": False, "cpu_baseline": True}
    assert not _legs(["--full", "--no-launch-timing"])["exclusive"]
    assert not _legs(["--full", "--data", "survey"])["continuity"]


def test_full_at_several_gpus_is_the_second_pass_alone():
    legs = _legs(["--gpus", "2", "--full"], world=2)
    assert legs["exclusive"] and not any(v for k, v in legs.items() if k != "exclusive")
