"""The environment variables of libswd_hip.so, from the source text alone (no library is loaded): csrc/swd_env.h holds the one table
and the one getenv, include/swd.h and INTEGRATION.md document exactly that table, and a variable is in the table if and only if a
file under tests/ or scripts/ sets it -- a switch nobody sets is deleted, not kept."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slidingwindowdecoder_amd", "csrc")

# read by Python itself (the package loader, bench.py, the tests and the fixture generators), never by the library
PYTHON_ONLY = {"SWD_LIB", "SWD_BENCH_STUB", "SWD_ORACLE_SO", "SWD_RECORD_REF", "SWD_FULL_GOLDEN",
               "SWD_GENERAL_SEARCH", "SWD_HEAVY_SEARCH", "SWD_NONFINITE_SEARCH", "SWD_REFBUILD"}  # (the last four: tests/golden/make_golden*.py)
PYTHON_ONLY_PREFIX = ("SWD_FUZZ_", "SWD_BENCH_")

# a name that is SET: monkeypatch.setenv / setdefault("NAME", ..), ["NAME"] = .., {"NAME": ..}, dict(.., NAME=..) and the shell's NAME=..
SET = re.compile(r"""set(?:env|default)\(\s*["'](SWD_[A-Z0-9_]+)["']|\[["'](SWD_[A-Z0-9_]+)["']\]\s*=(?!=)|["'](SWD_[A-Z0-9_]+)["']\s*:|\b(SWD_[A-Z0-9_]+)=(?!=)""")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _set_in(*patterns):
    """{name: [files that set it]} over the files the glob patterns (relative to the repository) name"""
    found = {}
    for pat in patterns:
        for path in glob.glob(os.path.join(ROOT, pat), recursive=True):
            if os.path.abspath(path) == os.path.abspath(__file__):
                continue
            for m in SET.finditer(_read(path)):
                found.setdefault(next(g for g in m.groups() if g), []).append(os.path.relpath(path, ROOT))
    return found


def _table():
    """the entries of SWD_ENV_TABLE: {name: (id, when, kind)}"""
    rows = re.findall(r'^\s*X\((\w+),\s*"(SWD_[A-Z0-9_]+)",\s*(\w+),\s*(\w+),\s*"[^"]+"\)', _read(os.path.join(CSRC, "swd_env.h")), re.M)
    assert rows and len({r[1] for r in rows}) == len(rows)
    for ident, name, when, kind in rows:
        assert name == "SWD_" + ident and when in ("PROCESS", "CREATE", "LAUNCH") and kind in ("PRESENT", "NONZERO", "INT", "STR"), name
    return {name: (ident, when, kind) for ident, name, when, kind in rows}


def test_one_getenv():
    """(a) the token getenv occurs in no file of csrc/ but swd_env.h"""
    users = [os.path.basename(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(p) and "getenv" in _read(p)]
    assert users == ["swd_env.h"]


def test_documents_list_the_table():
    """(b) the section of include/swd.h and the table of INTEGRATION.md name the variables of the table, all of them and no other --
    with the table's read time and value kind in the header"""
    table = _table()
    hdr = _read(os.path.join(ROOT, "include", "swd.h"))
    sec = hdr[hdr.index("Environment variables (test hooks and diagnostics)"):]
    sec = sec[:sec.index("*/")]
    assert set(re.findall(r"SWD_[A-Z0-9_]+", sec)) == set(table)
    rows = dict((n, (w, k)) for n, w, k in re.findall(r"^ \*   (SWD_[A-Z0-9_]+)\s+([PCL])\s+(set|nonzero|int|text)\s", sec, re.M))
    kinds = {"PRESENT": "set", "NONZERO": "nonzero", "INT": "int", "STR": "text"}
    assert rows == {n: (when[0], kinds[kind]) for n, (_, when, kind) in table.items()}
    doc = _read(os.path.join(ROOT, "INTEGRATION.md"))
    doc = doc[doc.index("Environment variables (diagnostics"):]
    cells = [line.split("|")[1] for line in doc.splitlines() if line.startswith("| `SWD_")]
    names = {n for c in cells for n in re.findall(r"SWD_[A-Z0-9_]+", c)}
    assert {n for n in names if n != "SWD_LIB" and not n.startswith("SWD_BENCH_")} == set(table)


def test_every_switch_the_tests_set_exists():
    """(c) what a test sets in os.environ or in a child's environment is in the table, or is read by Python itself"""
    table = _table()
    stray = {n: f for n, f in _set_in("tests/**/*.py").items()
             if n not in table and n not in PYTHON_ONLY and not n.startswith(PYTHON_ONLY_PREFIX)}
    assert not stray, f"set by a test, read by nobody: {stray}"


def test_every_switch_has_a_user():
    """(d) every entry of the table is set by a file under tests/ or scripts/"""
    used = _set_in("tests/**/*.py", "tests/**/*.sh", "scripts/**/*.py", "scripts/**/*.sh")
    unused = sorted(set(_table()) - set(used))
    assert not unused, f"no test or script sets {unused}: delete the switch (csrc/swd_env.h, include/swd.h, INTEGRATION.md)"
