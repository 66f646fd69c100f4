"""The build switches of the kernel sources, from the source text alone (nothing is compiled): the three kernel headers test only the
ten switches that choose code of the product or of an A/B build, every diagnostic switch is tested in csrc/swd_diag.h and nowhere
else (the headers use its one-line SWD_IF_<switch>(...) macros), DESIGN.md lists exactly the macros the conditionals under csrc/ test,
and the compile-time experiment switches that were folded out of swd_bp4_kernel.h stay out."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "slidingwindowdecoder_amd", "csrc")
KERNEL_HEADERS = ("swd_osdw_kernel.h", "swd_gdg_kernel.h", "swd_bp4_kernel.h")

KEPT = {"SWD_OSDW_TUNED", "SWD_TUNED_NT", "SWD_POST_DEPTH2", "SWD_POST_SORTED", "SWD_POST_KGP", "SWD_BIG_TBL", "SWD_BIG_REC",
        "SWD_QUAD_LAZY", "SWD_NO_SCALAR_ANY", "SWD_NO_SCALAR_WMAX"}
DIAGNOSTIC = {"SWD_BPPROF", "SWD_OSDPROF", "SWD_INITPROF", "SWD_SHPROF", "SWD_TSPROF", "SWD_SELPROF", "SWD_GDGPROF", "SWD_GDG_DEBUG",
              "SWD_GDG_CHECKS", "SWD_RESIDENCY", "SWD_BP4PROF"}
FOLDED_BP4 = ("SWD_BP4_CALLS", "SWD_BP4_OWN_CHECK", "SWD_BP4_ROLLED", "SWD_BP4_LAZY_MSG", "SWD_BP4_LAZY_ITS", "SWD_BP4_PRIO_IT",
              "SWD_BP4_WAVES", "SWD_BP4_WAVES_LAZY", "SWD_BP4_WAVES_LAZY8")

COUNTED = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef)\b", re.M)                      # what the caps count
CONDITION = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)          # ... and every line that tests a macro


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources():
    return sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p) and p.endswith((".h", ".hip")))


def _tested(text):
    """the macros the preprocessor conditionals of a file test; compiler macros (__HIPCC__, ...) are not the project's"""
    names = set()
    for cond in CONDITION.findall(text):
        cond = cond.split("//")[0]
        names |= {n for n in re.findall(r"[A-Za-z_]\w*", cond) if n != "defined" and not n.startswith("__")}
    return names


def test_kernel_headers_test_only_the_kept_switches():
    """(a) every conditional of the three kernel headers tests one of the ten kept switches; no file but swd_diag.h tests a
    diagnostic switch, and swd_diag.h tests nothing else"""
    for name in KERNEL_HEADERS:
        stray = _tested(_read(os.path.join(CSRC, name))) - KEPT
        assert not stray, f"{name} tests {sorted(stray)}: a diagnostic statement goes through SWD_IF_<switch>(...) of swd_diag.h"
    for path in _sources():
        tested = _tested(_read(path))
        if os.path.basename(path) == "swd_diag.h":
            assert tested == DIAGNOSTIC
        else:
            assert not tested & DIAGNOSTIC, f"{os.path.basename(path)} tests {sorted(tested & DIAGNOSTIC)}"


def test_conditional_counts_stay_low():
    """(b) conditionals per header"""
    caps = {"swd_osdw_kernel.h": 14, "swd_gdg_kernel.h": 0, "swd_bp4_kernel.h": 0, "swd_diag.h": len(DIAGNOSTIC) + 2}
    for name, cap in caps.items():
        n = len(COUNTED.findall(_read(os.path.join(CSRC, name))))
        assert n <= cap, f"{name}: {n} preprocessor conditionals, at most {cap}"


def test_every_diagnostic_macro_is_defined_once_per_branch():
    """swd_diag.h defines SWD_IF_<switch> in both branches of the switch's conditional, and the sources use no SWD_IF_ macro it
    does not define"""
    diag = _read(os.path.join(CSRC, "swd_diag.h"))
    defined = re.findall(r"^#define (SWD_IF_\w+)\(\.\.\.\)", diag, re.M)
    for sw in DIAGNOSTIC:
        assert defined.count("SWD_IF_" + sw[4:]) == 2, sw
    for path in _sources():
        used = set(re.findall(r"\bSWD_IF_[A-Z]\w*(?=\()", _read(path)))  # (SWD_IF_0 / SWD_IF_1: the variant lists' own SWD_IF(c, ...))
        assert used <= set(defined), f"{os.path.basename(path)}: {sorted(used - set(defined))}"


def test_design_table_lists_the_tested_macros():
    """(c) the macros any conditional under csrc/ tests are those of the table "Build switches of the pipeline kernels" in DESIGN.md"""
    tested = set()
    for path in _sources():
        tested |= _tested(_read(path))
    doc = _read(os.path.join(ROOT, "DESIGN.md"))
    doc = doc[doc.index("Build switches of the pipeline kernels"):]
    rows = []
    for line in doc.splitlines()[1:]:
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break
    listed = {n for row in rows for n in re.findall(r"`(SWD_[A-Z0-9_]+)`", row.split("|")[1])}
    assert listed == tested, f"only in DESIGN.md: {sorted(listed - tested)}; only in csrc/: {sorted(tested - listed)}"
    assert tested == KEPT | DIAGNOSTIC | {"SWD_HEADLINE_ONLY", "SWD_BB288_ONLY", "SWD_V7816_ONLY"}


def test_folded_bp4_switches_stay_out():
    """(d) no file under csrc/ names one of the nine compile-time experiment switches folded out of swd_bp4_kernel.h (the rejected
    forms are scripts/experiments/bp4_kernel_switches.patch)"""
    pat = re.compile(r"\b(?:%s)\b" % "|".join(FOLDED_BP4))
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path):
            with open(path, encoding="utf-8", errors="replace") as f:
                hits = sorted(set(pat.findall(f.read())))
            assert not hits, f"{os.path.basename(path)} names {hits}"
