"""Every example script of the reference checkout, imported UNMODIFIED under elodin_amd.compat in a process of its own (build
container only): which ones import, and — where the script calls `world.run(...)` at import — resolve to a program through
World.build; for seven of the traced ones the generated kernel is also compiled for gfx950 and must be register-resident.  A
regression list, not a parity test: the examples with reference-held data are pinned one by one in
tests/test_compat_reference_scripts.py.  The ones that cannot run here say why."""
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests import reference

REF = reference.under("examples")
ROOT = Path(__file__).resolve().parents[1]
pytestmark = pytest.mark.skipif(REF is None, reason=reference.SKIP_REASON)

ONE = r'''
import sys, importlib.util, os
sys.dont_write_bytecode = True
sys.path.insert(0, sys.argv[2]); sys.setrecursionlimit(50000)
import elodin_amd.compat as compat
compat.install(run="record", inert=("polars",))
path = sys.argv[1]
sys.path.insert(0, os.path.dirname(path))
spec = importlib.util.spec_from_file_location("ref_example", path)
m = importlib.util.module_from_spec(spec)
sys.modules["ref_example"] = m
spec.loader.exec_module(m)
worlds = [v for v in vars(m).values() if hasattr(v, "compat_run")]
if worlds:
    run = worlds[0].compat_run
    plan = worlds[0].build(run["system"], simulation_rate=run["simulation_rate"], telemetry_rate=run["telemetry_rate"], _dry=True)
    eff = plan["effectors"]
    if len(sys.argv) > 3 and hasattr(eff, "trace"):      # also generate + compile the program for gfx950 (hipcc cross-compiles)
        from elodin_amd import codegen
        codegen.build(eff.trace(), "float64", plan["integrator"])
        print("scratch", codegen.last_resources.get("scratch_bytes_per_lane"), "variant", codegen.last_variant[0])
    print("TRACED", len(eff.trace().columns) if hasattr(eff, "trace") else 0)
else:
    print("IMPORTED")
'''

# script -> what is expected of it: "traced" (runs its world at import: resolved to a program), "imported" (defines its world
# behind functions / __main__), or the reason it cannot get that far here
EXPECTED = {
    "apollo-lander/main.py": "traced", "ball/main.py": "imported", "covariance-ellipsoids/main.py": "imported",
    "crazyflie-edu/main.py": "traced", "drone/main.py": "traced", "ellipsoid/main.py": "imported", "f32-quant-repro/main.py": "imported",
    "frames/main.py": "imported", "geo-frames/main.py": "imported", "linalg/main.py": "traced", "logstream/main.py": "traced",
    "n-body/sim.py": "imported",              # main.py clears the example's database directory before it runs: sim.py only
    "rc-jet/main.py": "traced", "rocket-barrowman/main.py": "imported", "rotating-cube/main.py": "traced",
    "sensor-camera/main.py": "traced", "stablehlo/main.py": "traced", "terrain/main.py": "imported", "three-body/main.py": "traced",
    "video-stream/main.py": "traced",
    "cube-sat/main.py": "NotImplementedError",        # EGM08 gravity tables are a download (tests/cube_sat_util.py flies it with them replaced)
    "cube-sat-pysim/main.py": "NotImplementedError",  # same
    "falcon9/main.py": "traced",                      # the full mission world: 65 component columns (the limit is 128 since round 4); its ascent
                                                      # window is flown closed-loop on the reference's fixture in test_compat_reference_scripts.py
    "rocket/main.py": "traced",                       # polars subset (compat_polars), map_coordinates, the sample window spelled concatenate /
                                                      # lax.scan: pinned on its rocket-csv baseline in test_compat_reference_scripts.py
    "voyager/main.py": "spiceypy",                    # third-party ephemeris library, not in this image
    "db-client/main.py": "elodin.db",                 # a database client, no simulation
    "betaflight-sitl/main.py": "betaflight_SITL.elf",  # needs the Betaflight SITL binary (the script says so and exits)
    "monte-carlo/main.py": "traced",                  # its 262,144-row lookup table is a gather from device memory (dsl.gather); the
                                                      # campaign itself runs as one executor: tests/test_monte_carlo_example.py
}


# traced examples whose generated kernel is also compiled here (seconds each; linalg / drone / cube-sat / falcon9 have tests of their own)
COMPILED = ("apollo-lander/main.py", "crazyflie-edu/main.py", "logstream/main.py", "rc-jet/main.py", "sensor-camera/main.py",
            "stablehlo/main.py", "video-stream/main.py")


@pytest.mark.parametrize("script", sorted(EXPECTED))
def test_example_script_under_compat(script, tmp_path):
    want = EXPECTED[script]
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    extra = ["build"] if script in COMPILED else []
    r = subprocess.run([sys.executable, "-c", ONE, str(REF / script), str(ROOT), *extra], capture_output=True, text=True, timeout=900, cwd=tmp_path, env=env)
    last = (r.stdout.strip().splitlines() or [""])[-1]
    if want == "traced":
        assert r.returncode == 0 and last.startswith("TRACED"), (r.stdout[-300:], r.stderr[-600:])
        if script in COMPILED:      # register-resident on gfx950: no scratch, first variant
            assert "scratch 0 variant program" in r.stdout, r.stdout[-300:]
    elif want == "imported":
        assert r.returncode == 0 and last.startswith(("IMPORTED", "TRACED")), (r.stdout[-300:], r.stderr[-600:])
    else:
        assert r.returncode != 0 and want in r.stderr + r.stdout, (want, r.stdout[-300:], r.stderr[-600:])


def test_the_list_covers_every_example_with_a_script():
    have = {f"{d.name}/{f}" for d in REF.iterdir() if d.is_dir() for f in ("main.py",) if (d / f).exists()}
    assert have - set(EXPECTED) == {"n-body/main.py"}, have - set(EXPECTED)


def test_command_line_runner_in_record_mode(tmp_path):
    """`python -m elodin_amd.compat --record script.py`: the runner itself, without a GPU (world.run only records)."""
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-m", "elodin_amd.compat", "--record", str(REF / "three-body" / "main.py")],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    assert r.returncode == 0, r.stderr[-800:]
    r = subprocess.run([sys.executable, "-m", "elodin_amd.compat", str(REF / "three-body" / "no_such_script.py")],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)
    assert r.returncode != 0 and "no_such_script" in r.stderr
