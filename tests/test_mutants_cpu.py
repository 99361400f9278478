"""The patch set of tools/mutation_audit.py (tools/mutants/<library>/<name>.patch), checked without a GPU: a patch that no
longer applies, names an unknown library or touches more than its one file fails here, not in a GPU job."""
import importlib.util
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


AUDIT = _load("aqua_mutation_audit", os.path.join(ROOT, "tools", "mutation_audit.py"))
BUILD = _load("aqua_mutation_build", os.path.join(ROOT, "aquaticgymenv_amd", "build.py"))
PATCHES = AUDIT.patches()
IDS = ["%s/%s" % p[:2] for p in PATCHES]


def _known_libraries():
    """each_library() and the tables behind it: every name build.py's library() answers"""
    return set(BUILD.fifteen_libraries())


def test_every_patch_directory_is_a_library_the_tool_lists():
    on_disk = sorted(d for d in os.listdir(AUDIT.PATCHES) if os.path.isdir(os.path.join(AUDIT.PATCHES, d)))
    assert on_disk == sorted(AUDIT.LIBRARIES), "a directory under tools/mutants/ the tool would never look into"
    assert set(BUILD.each_library()) <= _known_libraries()
    for lib in AUDIT.LIBRARIES:
        assert lib in _known_libraries() and BUILD.library(lib)["src"], lib
        assert lib in AUDIT.FILES and AUDIT.FILES[lib], lib
        assert AUDIT.ENV[lib] == "AQUA_%s_LIB" % lib.upper()
        with open(os.path.join(ROOT, "aquaticgymenv_amd", "_%s_capi.py" % lib)) as f:
            assert '"%s"' % AUDIT.ENV[lib] in f.read(), "the binding reads another variable"


def test_the_audit_covers_thirteen_libraries_with_at_least_eight_mutants_each():
    assert len(AUDIT.LIBRARIES) == 13 and len(set(AUDIT.LIBRARIES)) == 13
    count = {lib: sum(1 for p in PATCHES if p[0] == lib) for lib in AUDIT.LIBRARIES}
    assert all(n >= 8 for n in count.values()), count
    assert len(set(IDS)) == len(IDS)


def test_every_test_file_the_audit_names_exists():
    for lib, files in AUDIT.FILES.items():
        for f in files:
            assert os.path.isfile(os.path.join(ROOT, f)), (lib, f)
    for f in AUDIT.NEW_FILES:
        assert os.path.isfile(os.path.join(ROOT, f)), f
    for lib in AUDIT.LIBRARIES:
        assert set(AUDIT.NEW_FILES_OF[lib]) <= set(AUDIT.NEW_FILES) and AUDIT.NEW_FILES_OF[lib], lib


@pytest.mark.parametrize("patch", PATCHES, ids=IDS)
def test_patch_is_described_and_touches_one_source_file(patch):
    lib, name, path, desc = patch
    with open(path) as f:
        lines = f.read().split("\n")
    assert desc and lines[0].strip() == desc and not desc.startswith(("---", "+++", "diff ", "@@")), "no description line"
    assert len(desc.split()) >= 3, "a description says what changes"
    old = [line.split()[1] for line in lines if line.startswith("--- ")]
    new = [line.split()[1] for line in lines if line.startswith("+++ ")]
    assert len(old) == 1 and len(new) == 1, (old, new)
    assert new[0].startswith("b/aquaticgymenv_amd/csrc/") and old[0] == "a/" + new[0][2:]
    target = new[0][2:]
    assert os.path.isfile(os.path.join(ROOT, target))
    # the file is one the library is built from: its own source, its header or a shared header it includes
    deps = [os.path.relpath(d, ROOT) for d in BUILD.library(lib)["deps"]]
    assert target in deps, (target, deps)
    AUDIT.check_patch(path)
    changed = [line for line in lines[1:] if line[:1] in "+-" and not line.startswith(("---", "+++"))]
    assert 1 <= len(changed) <= 12, "a mutant is a small diff"


@pytest.fixture(scope="module")
def scratch(tmp_path_factory):
    """a copy of csrc/ outside any repository"""
    if shutil.which("git") is None:
        pytest.skip("no git binary")
    top = tmp_path_factory.mktemp("mutants")
    shutil.copytree(os.path.join(ROOT, "aquaticgymenv_amd", "csrc"), str(top / "aquaticgymenv_amd" / "csrc"))
    return str(top)


@pytest.mark.parametrize("patch", PATCHES, ids=IDS)
def test_patch_applies_to_the_sources_as_they_are(scratch, patch):
    lib, name, path, desc = patch
    env = dict(os.environ, GIT_CEILING_DIRECTORIES=os.path.dirname(scratch))
    r = subprocess.run(["git", "apply", "--check", "--verbose", path], cwd=scratch, capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stderr


def test_collect_merges_and_keeps_the_records_it_does_not_rerun(tmp_path, monkeypatch):
    """--collect with one fresh run: that record is replaced, every other one stays what it was"""
    import json
    with open(AUDIT.RECORD) as f:
        before = json.load(f)
    record = str(tmp_path / "record.json")
    shutil.copy(AUDIT.RECORD, record)
    out = tmp_path / "runs" / "policy"
    out.mkdir(parents=True)
    with open(str(out / "explore_le.json"), "w") as f:
        json.dump({"library": "policy", "mutant": "explore_le", "tests": 3, "failing_before": ["tests.test_a::x[1]", "tests.test_a::x[2]"],
                   "failing_new": ["tests.test_b::y"]}, f)
    monkeypatch.setattr(AUDIT, "RECORD", record)
    monkeypatch.setattr(AUDIT, "OUT_RUNS", str(tmp_path / "runs"))
    assert AUDIT.cmd_collect() == 0
    with open(record) as f:
        after = json.load(f)
    old = {(m["library"], m["mutant"]): m for m in before["mutants"]}
    new = {(m["library"], m["mutant"]): m for m in after["mutants"]}
    assert set(old) <= set(new)
    for key, m in old.items():
        if key == ("policy", "explore_le"):
            assert new[key]["failing_before"] == 2 and new[key]["failing_after"] == 3 and new[key]["tests_run"] == 3
            assert new[key]["killed_by_before"] == ["test_a::x"] and new[key]["killed_by_new"] == ["test_b::y"]
        else:
            assert new[key] == m, key
