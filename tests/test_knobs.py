"""The environment knobs live in one table (openr_amd/csrc/common/knobs.h).

No GPU, no native library: the checks read source text only.
  (a) nothing under openr_amd/csrc reads the environment except that header;
  (b) every OSPF_* / ODL_* knob named by a test, the benchmark, a script, a
      public header, INTEGRATION.md or DESIGN.md's knob table is in the table
      (a misspelt knob in a test would silently test the default);
  (c) DESIGN.md's knob table lists every knob of the header.
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "openr_amd", "csrc")
KNOBS_H = os.path.join(CSRC, "common", "knobs.h")
TOKEN = re.compile(r"\b(?:OSPF|ODL)_[A-Z0-9_]+")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _table():
    """{name: kind} from the header's X-macro lines."""
    rows = re.findall(r"^\s*X\((\w+),\s*(SET|NONZERO|INT|STR),", _read(KNOBS_H), re.M)
    assert len(rows) > 50 and len({n for n, _ in rows}) == len(rows)
    return dict(rows)


def _abi_constants():
    """Macros and enumerators of the public headers that share the knobs' prefixes."""
    out = set()
    for h in glob.glob(os.path.join(ROOT, "include", "*.h")):
        text = _read(h)
        out |= set(re.findall(r"^\s*#\s*define\s+((?:OSPF|ODL)_[A-Z0-9_]+)", text, re.M))
        for body in re.findall(r"\benum\b[^{;]*\{([^}]*)\}", text):
            out |= set(TOKEN.findall(re.sub(r"/\*.*?\*/|//[^\n]*", "", body, flags=re.S)))
    assert "OSPF_OK" in out and "OSPF_WANT_NH" in out and "OSPF_SWEEP_DEFER" in out
    return out


def _design_table():
    """Knob names of DESIGN.md's knob section: the first cell of each table row."""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## 9\. Environment knobs\n(.*?)(?=^## |\Z)", text, re.M | re.S)
    assert m, "DESIGN.md has no '## 9. Environment knobs' section"
    return re.findall(r"^\| `(\w+)` \|", m.group(1), re.M), m.group(1)


def test_getenv_only_in_knob_header():
    hits = []
    for path in glob.glob(os.path.join(CSRC, "**", "*"), recursive=True):
        if os.path.isfile(path) and os.path.abspath(path) != KNOBS_H and "getenv(" in _read(path):
            hits.append(os.path.relpath(path, ROOT))
    assert not hits, f"getenv( outside knobs.h: {hits}"


def test_every_named_knob_is_in_the_table():
    table, abi = _table(), _abi_constants()
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + [os.path.join(ROOT, "bench.py")]
    files += [p for p in glob.glob(os.path.join(ROOT, "scripts", "**", "*"), recursive=True)
              if os.path.isfile(p)]
    files += glob.glob(os.path.join(ROOT, "include", "*.h"))
    files.append(os.path.join(ROOT, "INTEGRATION.md"))
    unknown = {}
    for path in files:
        for tok in set(TOKEN.findall(_read(path))):
            if tok.endswith("_"):  # a prefix in prose, as in OSPF_E_*
                continue
            if tok not in table and tok not in abi:
                unknown.setdefault(tok, []).append(os.path.relpath(path, ROOT))
    _, section = _design_table()
    rows = "\n".join(ln for ln in section.splitlines() if ln.startswith("|"))
    for tok in set(TOKEN.findall(rows)):
        if not tok.endswith("_") and tok not in table and tok not in abi:
            unknown.setdefault(tok, []).append("DESIGN.md §9")
    assert not unknown, f"names that are neither a knob of knobs.h nor an ABI constant: {unknown}"


def test_design_lists_every_knob():
    table = _table()
    listed, _ = _design_table()
    assert listed == list(table), (
        f"DESIGN.md §9 differs from knobs.h: missing {sorted(set(table) - set(listed))}, "
        f"extra {sorted(set(listed) - set(table))}, or another order")
