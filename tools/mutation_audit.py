#!/usr/bin/env python
"""Mutation audit of thirteen device libraries: does the GPU suite bite?

First audit: policy, bank, episodes, replay, learner.  Second audit: lbank, segments, pbt, qmap, fastpol, nstep, prio, her.

A mutant is a patch tools/mutants/<library>/<name>.patch: a one-line description, then a small unified diff against ONE
file under aquaticgymenv_amd/csrc/.  Mutant libraries and the scratch trees they are built in are never committed.

THE RULE FOR MUTANTS (enforced by review).  Each mutant changes the VALUE of one arithmetic expression, constant or value
comparison.  None changes an index, an address, a bound on an index, a loop trip count, a barrier or fence, an LDS layout,
a launch shape or an argument check.  A mutant must be unable to read or write where the shipped kernel does not: the aim
is a failing assertion, never a fault.  A value that later selects a slot (the k of a relabelling draw, a window limit) is
mutated only where the mutated arithmetic itself still proves the range, and the patch's description line says why.

  --build [LIB[/NAME] ...]   for every patch: copy csrc/, include/ and build.py into a scratch tree of its own (never the
                             working tree), apply the patch there (one that no longer applies is an error and the exit
                             status is 2), build that one library with the project's recipe (build.py: its table entry of
                             each_library(), cross-compiled for gfx950, no GPU needed) and put the result at
                             gpu_jobs/mutants/<library>/<name>.so (a folder that travels to the GPU machine and stays
                             out of git).
  --run LIB/NAME             one pytest child over the GPU test files of that library (FILES below) and, of the file
                             its audit added, the cases named for that library (selection_of) with the mutant
                             substituted through the variable the binding's lib_path() honours; writes
                             <out>/<library>/<name>.json, .xml and .log.  Exit status 0: survived, 1: killed; anything
                             else (a crash of the child, a HIP error text in its log) is passed on as a status >= 2 and
                             the caller must stop: read what it left before anything else runs on the GPU.  No retries.
  --list                     LIB/NAME of every patch, one per line (what a job script loops over)
  --collect                  <out>/**.json -> profiles/mutation_audit.json and the tables for profiles/LOG.md on stdout.
                             It MERGES: a mutant without a run under <out> keeps the record it has, bit for bit
  --out DIR                  where --run writes and --collect reads (default build/mutation, which git ignores): a job on
                             another machine names a folder whose contents come back from it

"before" counts failures in the test files that existed before the audit, "after" adds the files written for what it
found (NEW_FILES): one run per mutant gives both columns.
"""
import argparse
import concurrent.futures
import glob
import importlib.util
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import xml.etree.ElementTree as ET

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCHES = os.path.join(ROOT, "tools", "mutants")
OUT_LIBS = os.path.join(ROOT, "gpu_jobs", "mutants")
OUT_RUNS = os.path.join(ROOT, "build", "mutation")          # --out replaces it
RECORD = os.path.join(ROOT, "profiles", "mutation_audit.json")

LIBRARIES = ("policy", "bank", "episodes", "replay", "learner",                    # the first audit
             "lbank", "segments", "pbt", "qmap", "fastpol", "nstep", "prio", "her")   # the second
ENV = {lib: "AQUA_%s_LIB" % lib.upper() for lib in LIBRARIES}              # what _<lib>_capi.py hands to _loader.lib_path()
TRAINER = "tests/test_trainer_gpu.py"
FILES = {                                                                  # the GPU test files of a library, before the audit
    "policy": ["tests/test_qpolicy_gpu.py"],
    "bank": ["tests/test_qbank_gpu.py"],
    "episodes": ["tests/test_episodes_gpu.py", TRAINER],
    "replay": ["tests/test_replay_gpu.py", TRAINER],
    "learner": ["tests/test_learner_gpu.py", "tests/test_learner_forms_gpu.py", TRAINER],
    # the second audit: each of these files also holds the loop tests (DQNLoop / PopulationLoop) that run its library
    "lbank": ["tests/test_lbank_gpu.py"],
    "segments": ["tests/test_segments_gpu.py"],
    "pbt": ["tests/test_pbt_gpu.py"],
    "qmap": ["tests/test_qmaps_gpu.py"],
    "fastpol": ["tests/test_fastpol_gpu.py"],
    "nstep": ["tests/test_nstep_gpu.py"],
    "prio": ["tests/test_prio_gpu.py"],
    "her": ["tests/test_her_gpu.py"],
}
# what the audits added: the "after" column
NEW_FILES = ["tests/test_dqn_knife_gpu.py", "tests/test_dqn_poison_gpu.py", "tests/test_population_knife_gpu.py"]
FIRST_AUDIT = LIBRARIES[:5]
NEW_FILES_OF = {lib: (NEW_FILES[:2] if lib in FIRST_AUDIT else NEW_FILES[2:]) for lib in LIBRARIES}   # an audit's own new files
HIP_ERROR = re.compile(r"HIP error|hipError|illegal memory access|Memory access fault|HSA_STATUS_ERROR", re.I)


def files_of(lib):
    """the test files one --run of a mutant of `lib` goes over: the library's own, then what its audit added (if it exists yet)"""
    return FILES[lib] + [f for f in NEW_FILES_OF[lib] if os.path.exists(os.path.join(ROOT, f))]


def selection_of(lib):
    """pytest arguments that keep, of the second audit's knife file, the cases of `lib` alone (they are named
    test_<lib>_...; the other libraries are the shipped ones in this run, their cases could only pass): [] for the first audit"""
    if lib in FIRST_AUDIT:
        return []
    return ["-k", "not (%s)" % " or ".join("test_%s_" % other for other in LIBRARIES if other not in FIRST_AUDIT and other != lib)]


def patches(selection=()):
    """-> [(library, name, path, description)] of every committed patch, or of those `selection` (LIB or LIB/NAME) names"""
    out = []
    for lib in LIBRARIES:
        for path in sorted(glob.glob(os.path.join(PATCHES, lib, "*.patch"))):
            name = os.path.basename(path)[:-len(".patch")]
            if selection and lib not in selection and "%s/%s" % (lib, name) not in selection:
                continue
            with open(path) as f:
                out.append((lib, name, path, f.readline().strip()))
    return out


def check_patch(path):
    """one file under aquaticgymenv_amd/csrc/, nothing else"""
    with open(path) as f:
        targets = [line.split()[1] for line in f if line.startswith("+++ ")]
    if len(targets) != 1 or not targets[0].startswith("b/aquaticgymenv_amd/csrc/"):
        raise SystemExit("%s: a mutant patches exactly one file under aquaticgymenv_amd/csrc/, found %r" % (path, targets))


def build_one(lib, name, path):
    """-> (LIB/NAME, None) or (LIB/NAME, what went wrong)"""
    what = "%s/%s" % (lib, name)
    check_patch(path)
    scratch = tempfile.mkdtemp(prefix="aqua_mutant_%s_%s_" % (lib, name))
    try:
        pkg = os.path.join(scratch, "aquaticgymenv_amd")
        os.makedirs(pkg)
        shutil.copytree(os.path.join(ROOT, "aquaticgymenv_amd", "csrc"), os.path.join(pkg, "csrc"))
        shutil.copytree(os.path.join(ROOT, "include"), os.path.join(scratch, "include"))
        if os.path.isdir(os.path.join(ROOT, "aquaticgymenv_amd", "include")):      # the headers of the package's own libraries
            shutil.copytree(os.path.join(ROOT, "aquaticgymenv_amd", "include"), os.path.join(pkg, "include"))
        shutil.copy(os.path.join(ROOT, "aquaticgymenv_amd", "build.py"), pkg)
        # git apply outside a repository is a strict `patch`: no fuzz, and text in front of the diff is skipped
        r = subprocess.run(["git", "apply", "--verbose", path], cwd=scratch, capture_output=True, text=True)
        if r.returncode != 0:
            return what, "the patch no longer applies:\n" + r.stderr
        spec = importlib.util.spec_from_file_location("aqua_mutant_build_%s_%s" % (lib, name), os.path.join(pkg, "build.py"))
        build = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(build)
        try:                                                        # (each_library() ends at the bank: library() looks in every table)
            build.library(lib)
        except KeyError:
            return what, "build.py knows no library %r" % lib
        try:
            built = build.build_library(lib, force=True)
        except subprocess.CalledProcessError as e:
            return what, "the mutant does not compile: %s" % e
        dst = os.path.join(OUT_LIBS, lib, name + ".so")
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        shutil.copy(built, dst)
        return what, None
    finally:
        shutil.rmtree(scratch, ignore_errors=True)


def cmd_build(selection, jobs):
    todo = patches(selection)
    if not todo:
        raise SystemExit("no patch matches %r" % (selection,))
    failed = []
    with concurrent.futures.ThreadPoolExecutor(max_workers=jobs) as pool:
        for what, err in pool.map(lambda t: build_one(*t[:3]), todo):
            print("%-40s %s" % (what, "built" if err is None else "FAILED"), flush=True)
            if err is not None:
                failed.append((what, err))
    for what, err in failed:
        print("\n%s: %s" % (what, err), file=sys.stderr)
    print("%d of %d mutant libraries under %s" % (len(todo) - len(failed), len(todo), os.path.relpath(OUT_LIBS, ROOT)))
    return 2 if failed else 0


def cmd_run(what):
    lib, name = what.split("/")
    so = os.path.join(OUT_LIBS, lib, name + ".so")
    if not os.path.exists(so):
        raise SystemExit("%s is not built: --build %s" % (os.path.relpath(so, ROOT), what))
    out_dir = os.path.join(OUT_RUNS, lib)
    os.makedirs(out_dir, exist_ok=True)
    xml, log = os.path.join(out_dir, name + ".xml"), os.path.join(out_dir, name + ".log")
    files = files_of(lib)
    env = dict(os.environ)
    env[ENV[lib]] = so
    cmd = [sys.executable, "-m", "pytest", "-q", "-m", "gpu", "-p", "no:cacheprovider", "--tb=line", "--junitxml", xml] + selection_of(lib) + files
    with open(log, "w") as f:
        rc = subprocess.run(cmd, cwd=ROOT, env=env, stdout=f, stderr=subprocess.STDOUT).returncode
    with open(log) as f:
        text = f.read()
    if HIP_ERROR.search(text):
        print("%s: a HIP error text in %s: stop and read it" % (what, os.path.relpath(log, ROOT)))
        return 3
    if rc not in (0, 1):
        print("%s: pytest ended with status %d, see %s" % (what, rc, os.path.relpath(log, ROOT)))
        return rc if rc >= 2 else 4
    before, after, total = [], [], 0
    for case in ET.parse(xml).getroot().iter("testcase"):
        total += 1
        if case.find("failure") is not None or case.find("error") is not None:
            test = "%s::%s" % (case.get("classname"), case.get("name"))
            (after if any(test.startswith(f[:-3].replace("/", ".")) for f in NEW_FILES) else before).append(test)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump({"library": lib, "mutant": name, "tests": total, "failing_before": sorted(before), "failing_new": sorted(after)}, f, indent=1)
    print("%-40s %s: %d of the earlier tests fail, %d of the new ones (of %d run)"
          % (what, "killed" if rc else "SURVIVED", len(before), len(after), total), flush=True)
    return rc


def cmd_collect():
    record, missing, kept = {"files": FILES, "new_files": NEW_FILES, "mutants": []}, [], {}
    if os.path.exists(RECORD):                                      # merge: what is not re-run keeps its record
        with open(RECORD) as f:
            kept = {(m["library"], m["mutant"]): m for m in json.load(f)["mutants"]}
    for lib, name, path, desc in patches():
        run = os.path.join(OUT_RUNS, lib, name + ".json")
        if not os.path.exists(run):
            if (lib, name) in kept:
                record["mutants"].append(kept[(lib, name)])
            else:
                missing.append("%s/%s" % (lib, name))
            continue
        with open(run) as f:
            r = json.load(f)
        short = lambda ids: sorted({i.split("::")[0].split(".")[-1] + "::" + i.split("::")[1].split("[")[0] for i in ids})     # noqa: E731
        record["mutants"].append({"library": lib, "mutant": name, "description": desc, "tests_run": r["tests"],
                                  "failing_before": len(r["failing_before"]), "failing_after": len(r["failing_before"]) + len(r["failing_new"]),
                                  "killed_by_before": short(r["failing_before"]), "killed_by_new": short(r["failing_new"])})
    with open(RECORD, "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")
    for lib in LIBRARIES:
        print("\n`libaqua_%s.so` (%s):\n" % (lib, " + ".join("`%s`" % f for f in FILES[lib])))
        print("| mutant | failing before | failing after |\n|---|---|---|")
        for m in record["mutants"]:
            if m["library"] == lib:
                print("| `%s`: %s | %d | %d%s |" % (m["mutant"], m["description"], m["failing_before"], m["failing_after"],
                                                     " (%s)" % ", ".join(n.split("::")[1] for n in m["killed_by_new"]) if m["killed_by_new"] else ""))
    if missing:
        print("\nnot run: " + " ".join(missing), file=sys.stderr)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--build", nargs="*", metavar="LIB[/NAME]")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--run", metavar="LIB/NAME")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--collect", action="store_true")
    ap.add_argument("--out", metavar="DIR", default=None)
    args = ap.parse_args()
    if args.out:
        global OUT_RUNS
        OUT_RUNS = os.path.abspath(args.out)
    if args.list:
        print("\n".join("%s/%s" % p[:2] for p in patches()))
        return 0
    if args.build is not None:
        return cmd_build(tuple(args.build), args.jobs)
    if args.run:
        return cmd_run(args.run)
    if args.collect:
        return cmd_collect()
    ap.print_help()
    return 2


if __name__ == "__main__":
    sys.exit(main())
