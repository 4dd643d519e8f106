"""Records which kernels a render launches, with which geometry: the inventory tests/golden/launch_inventory.json that the launch choice
(tungsten_amd/csrc/host/LaunchChoice.cpp) and the context's launch plan are held to.  Needs a GPU and rocprofv3.

    python tools/launch_inventory.py --record out.json [--only SCENE ...]
    python tools/launch_inventory.py --render SCENE_FILE key=value ...          (what --record traces, one process per case)

Per case of tests/launch_cases.py: one `rocprofv3 --kernel-trace` of one render -- no counters, no other tracing, a time limit of its own --, reduced to
the distinct (kernel, workgroup size, LDS bytes, grid size) of the launch families the choice decides with the number of such launches, kernel names in the
canonical spelling of kernelName(); and, from the library's TGHIP_VERBOSE lines, the kinds of passes the render ran (flags, short or not).  The first case that fails ends
the run.  LDS bytes are what the trace reports: the kernel's static LDS in units of 512 bytes (a kernel trace does not show a launch's dynamic bytes).

Every render runs with "check_interval" = 1 and "tail_threshold" = 256 next to the case's options: at the goldens' sizes a pass starts below the default
threshold and would run in k_tail alone; so the loop's kernels run first and k_tail ends the pass where the choice allows it."""
import argparse
import collections
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

BASE_OPTIONS = {"check_interval": 1, "tail_threshold": 256}
# the launch families the choice decides (k_start, k_finish, k_resolve ... are launched whatever the scene)
CHOSEN = re.compile(r"^(k_trace_closest|k_finish_trace_closest_wide|k_trace_shadow|k_shade|k_tail|k_camera_rays)")
TIME_LIMIT = 180


def canonical(name):
    """`void k_shade<8195u, 2, 7, false>(DeviceScene, PathState, PassParams, int) [clone .kd]` -> `k_shade<8195,2,7,false>`"""
    name = re.sub(r"\s*\[clone[^\]]*\]", "", name).strip()
    name = re.sub(r"^void\s+", "", name)
    name = re.sub(r"\(.*\)$", "", name)
    name = re.sub(r"(\d)u\b", r"\1", name.replace(" ", ""))
    return re.sub(r"\.kd$", "", name)


def render(scene_file, options):
    import tungsten_amd as tg
    r = tg.Renderer(scene_file, seed=tg.DEFAULT_SEED)
    for k, v in options.items():
        r.set_option(k, v)
    r.render()
    r.close()


def trace(case, scene_file, options, out_dir):
    """One traced render: ({(kernel, wg, lds, grid): calls}, sorted [(flags, short)]) or None when the process failed."""
    os.makedirs(out_dir, exist_ok=True)
    args = ["%s=%d" % kv for kv in sorted(dict(BASE_OPTIONS, **options).items())]
    cmd = ["timeout", "-k", "10", str(TIME_LIMIT), "rocprofv3", "--kernel-trace", "-f", "csv", "-d", out_dir, "-o", "trace", "--",
           sys.executable, os.path.abspath(__file__), "--render", scene_file] + args
    proc = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, TGHIP_VERBOSE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    if proc.returncode != 0:
        sys.stderr.write("%s: exit status %d\n%s\n" % (case, proc.returncode, proc.stderr[-3000:]))
        return None
    passes = sorted({(int(m.group(1)), int(m.group(2))) for m in re.finditer(r"\[tghip\] pass spp \[\d+, \d+\) flags (\d+):.*? short (\d)", proc.stderr)})
    files = glob.glob(os.path.join(out_dir, "**", "*kernel_trace.csv"), recursive=True)
    if len(files) != 1:
        sys.stderr.write("%s: %d kernel traces under %s\n" % (case, len(files), out_dir))
        return None
    launches = collections.Counter()
    with open(files[0], newline="") as f:
        for row in csv.DictReader(f):
            name = canonical(row["Kernel_Name"])
            if CHOSEN.match(name):
                launches[(name, int(row["Workgroup_Size_X"]), int(row["LDS_Block_Size"]), int(row["Grid_Size_X"])//int(row["Workgroup_Size_X"]))] += 1
    return launches, passes


def record(out_json, only):
    import tungsten_amd as tg
    import launch_cases
    inventory = collections.OrderedDict()
    with tempfile.TemporaryDirectory(prefix="launch_inventory_") as tmp:
        for case, scene, options, path in launch_cases.cases(os.path.join(tmp, "scenes"), tg.lib):
            if only and scene not in only:
                continue
            got = trace(case, path, options, os.path.join(tmp, "traces", re.sub(r"[^A-Za-z0-9_]", "_", case)))
            if got is None:
                return 1
            launches, passes = got
            inventory[case] = {"scene": scene, "options": options, "passes": [list(p) for p in passes], "launches": [list(k) + [n] for k, n in sorted(launches.items())]}
            print("%s: %d passes kinds, %d distinct launches" % (case, len(passes), len(launches)), flush=True)
    with open(out_json, "w") as f:                                     # (one case per line)
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in inventory.items()) + "\n}\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record")
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--render", nargs="+")
    a = ap.parse_args()
    if a.render:
        render(a.render[0], {k: int(v) for k, v in (kv.split("=") for kv in a.render[1:])})
        return 0
    return record(a.record, a.only)


if __name__ == "__main__":
    sys.exit(main())
