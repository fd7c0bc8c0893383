"""bench.py's command line (CPU): --full exists and is off by default, and the project's own scripts that keep what only
--full measures (the legs, the per-half pass, the line without the check) ask for it."""
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_is_an_option_and_off_by_default():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert re.search(r'add_argument\("--full", action="store_true"', src)      # store_true: False unless given


def test_profile_scripts_ask_for_the_full_line():
    """The scripts whose output is committed under profiles/ (bench lines with legs and CPU baseline, kernel statistics and
    counters over every launch of the process) run the benchmark with --full wherever they fix its arguments themselves."""
    for name in ("profile_round.sh", "profile_workload.sh", "pmc_quick.sh", "pmc_traffic_quick.sh"):
        calls = [ln for ln in open(os.path.join(ROOT, "tools", name)) if "bench.py" in ln and not ln.lstrip().startswith("#")]
        assert calls, name
        assert all(re.search(r"bench\.py --full\b", ln) for ln in calls), (name, [ln[:120] for ln in calls if "--full" not in ln])
