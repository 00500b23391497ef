#!/usr/bin/env python3
"""Which test file launches which compiled kernel: joins rocprofv3 kernel statistics with tests/kernel_catalogue.py.

  kernel_coverage.py steps
      one line per profiler step, "<name>\t<pytest arguments>":
        a_<file>  the new catalogue GPU file, and per file the `covered_by` / `exempt` tests the catalogue names;
        b_<file>  every reference-checking GPU file as the parent commit has it, without the tests that start child processes
                  (the -k expression LEFT_OUT below).
      A job script runs each step as
        timeout -k 10 <s> rocprofv3 --kernel-trace --stats --output-format csv -d <dir>/<name> -- python -m pytest <arguments>
      (no counters, no other tracing), keeps <dir>/<name>/**/*kernel_stats.csv as <out>/<name>_kernel_stats.csv and writes
      "<name> <exit status> <seconds>" lines to <out>/steps*.txt.  A step whose status is not 0 is "not traced" and is not run again.

  kernel_coverage.py ledger <out> [ledger file]
      writes profiles/kernel_coverage.txt: per kernel the files that launched it before (b) and after (a) this catalogue, the
      kernels no parent file launched (the measured gap), and whether (a) launched everything the catalogue says it does;
      the lines of <out>/times.txt, if there, are copied in as "running times".
      Exit status 1 when (a) misses a catalogued kernel or launches one without a record.

Only kernel names are read from the profiler's tables."""
import csv
import glob
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import kernel_catalogue as kc     # noqa: E402

NEW_FILE = "tests/test_gpu_kernel_catalogue.py"
# every GPU test that starts a child process (bench.py, the distributed drivers, the C clients, the command line as a program)
LEFT_OUT = ("bench or nccl or c_client or launcher or without_torch or three_ranks or rccl_merge_path_world or "
            "reads_no_environment_switch or wav_file or resamples_the_audio")


def parent_files():
    return sorted("tests/" + os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py"))
                  if os.path.basename(p) != os.path.basename(NEW_FILE))


def step_name(prefix, path):
    return prefix + "_" + os.path.basename(path)[len("test_gpu_"):-3]


def steps():
    out = [(step_name("a", NEW_FILE), [NEW_FILE])]
    named = {}
    for r in kc.RECORDS:
        for node in r.get("covered_by", ()) + ((r["exempt"],) if "exempt" in r else ()):
            named.setdefault(node.split("::")[0], set()).add(node)
    out += [(step_name("a", path), sorted(nodes)) for path, nodes in sorted(named.items())]
    out += [(step_name("b", path), [path, "-k", "not (%s)" % LEFT_OUT]) for path in parent_files()]
    return [(name, ["-m", "gpu", "-q", "-p", "no:cacheprovider"] + args) for name, args in steps_sorted(out)]


def steps_sorted(items):
    return sorted(items, key=lambda it: it[0])


def traced_kernels(path):
    """Short kernel names of one *_kernel_stats.csv (the profiler's "Name" column holds demangled names)."""
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    raw = sorted({re.sub(r"\.kd$", "", (row.get("Name") or row.get("Kernel_Name") or row.get("KernelName") or "").strip()) for row in rows})
    mangled = [n for n in raw if n.startswith("_Z")]
    if mangled:
        plain = subprocess.run(["c++filt"] + mangled, capture_output=True, text=True).stdout.split("\n")
        raw = [n for n in raw if not n.startswith("_Z")] + plain[:len(mangled)]
    return {kc.short_name(n) for n in raw if kc.short_name(n).startswith("ksa::")}


def left_out_tests():
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-m", "gpu", "-p", "no:cacheprovider", "-k", LEFT_OUT] + parent_files(),
                       cwd=ROOT, capture_output=True, text=True)
    return sorted({re.sub(r"\[.*", "", line.strip()) for line in r.stdout.splitlines() if "::" in line})


def ledger(out_dir, target):
    status = {}
    for steps_file in sorted(glob.glob(os.path.join(out_dir, "steps*.txt"))):
        for line in open(steps_file):
            name, rc, secs = line.split()[:3]
            status[name] = (int(rc), float(secs))
    launched = {}                  # step -> names
    for name, _ in steps():
        path = os.path.join(out_dir, name + "_kernel_stats.csv")
        if status.get(name, (None,))[0] == 0 and os.path.exists(path):
            launched[name] = traced_kernels(path)
    table = {r["kernel"]: r for r in kc.RECORDS}
    after = set().union(*[v for k, v in launched.items() if k.startswith("a_")] or [set()])
    before = set().union(*[v for k, v in launched.items() if k.startswith("b_")] or [set()])
    expected = {k for k, r in table.items() if kc.kind_of(r) in ("recipe", "covered_by")}
    exempt = {k for k, r in table.items() if kc.kind_of(r) == "exempt"}
    missing, unknown = sorted(expected - after), sorted(after - set(table))
    own = launched.get(step_name("a", NEW_FILE), set())           # a recipe must be launched by the catalogue file itself
    missing += sorted(k + " (its recipe did not launch it)" for k, r in table.items() if kc.kind_of(r) == "recipe" and k in after and k not in own)
    gap = sorted(k for k in expected if k not in before)
    lines = ["Kernel coverage ledger: tests/kernel_catalogue.py joined with rocprofv3 --kernel-trace --stats (tools/kernel_coverage.py).",
             "%d records: %d recipe, %d covered_by, %d exempt, %d unreachable." % (
                 len(table), *[sum(kc.kind_of(r) == k for r in table.values()) for k in kc.KINDS]), "",
             "steps (exit status, seconds under the profiler; a status other than 0 is NOT TRACED and was not run again):"]
    for name, _ in steps():
        rc, secs = status.get(name, (None, 0.0))
        lines.append("  %-24s %s" % (name, "not run" if rc is None else "%d  %6.1f s%s" % (rc, secs, "" if rc == 0 else "  NOT TRACED")))
    times = os.path.join(out_dir, "times.txt")           # free text: the running times measured in the same session
    if os.path.exists(times):
        lines += ["", "running times:"] + ["  " + t.rstrip() for t in open(times)]
    lines += ["", "left out of (b), tests that start child processes (-k \"not (%s)\"):" % LEFT_OUT]
    lines += ["  " + t for t in left_out_tests()]
    lines += ["", "(a) launched %d of the %d kernels with a recipe or covered_by record%s" % (
        len(expected & after), len(expected), "; the exempt kernel%s launched" % (" was" if exempt <= after else " was NOT"))]
    lines += ["  MISSING from (a): " + k for k in missing] + ["  launched by (a) WITHOUT a record: " + k for k in unknown]
    lines += ["", "kernels no parent GPU file launched (b): %d" % len(gap)] + ["  " + k for k in gap]
    lines += ["", "per kernel: files that launched it before (b) | after (a)"]
    for k in sorted(table):
        b = sorted(s[2:] for s, v in launched.items() if s.startswith("b_") and k in v)
        a = sorted(s[2:] for s, v in launched.items() if s.startswith("a_") and k in v)
        lines.append("  %-60s %-12s %s | %s" % (k, kc.kind_of(table[k]), ",".join(b) or "-", ",".join(a) or "-"))
    with open(target, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines[:12 + len(steps())]))
    print("gap %d, missing %d, unknown %d -> %s" % (len(gap), len(missing), len(unknown), target))
    return 1 if missing or unknown else 0


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "steps":
        for name, args in steps():
            print(name + "\t" + " ".join("'%s'" % a if " " in a else a for a in args))
    elif len(sys.argv) >= 3 and sys.argv[1] == "ledger":
        sys.exit(ledger(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "kernel_coverage.txt")))
    else:
        sys.exit(__doc__)
