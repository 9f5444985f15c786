"""The DISYOLO_* environment switches the product reads are exactly those of DESIGN.md's table (section 7b): a switch that
comes back, or a new one, has to be written down there -- with its default, its reader and its purpose -- to exist."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = r"(DISYOLO_[A-Z0-9_]+)"
# os.environ[...] / .get / .setdefault / .pop, os.getenv(...), a bare ``environ`` imported from os, and ``"NAME" in os.environ``
PY_READ = re.compile(r"(?:\benviron(?:\.get|\.setdefault|\.pop)?\s*[\(\[]|\bgetenv\s*\()\s*[\"']" + NAME)
PY_IN = re.compile(r"[\"']" + NAME + r"[\"']\s+(?:not\s+)?in\s+(?:_?os\.)?environ")
# in csrc every string literal that is exactly a switch name counts, not only getenv's argument: a helper that takes the name
# (an env_int("DISYOLO_X", 1)) is a read too.  Comments are stripped first.
C_COMMENT = re.compile(r"//[^\n]*|/\*.*?\*/", re.S)
C_NAME = re.compile(r"\"" + NAME + r"\"")


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _python_names(text):
    return set(PY_READ.findall(text)) | set(PY_IN.findall(text))


def _source_names():
    names = set()
    for path in glob.glob(os.path.join(ROOT, "dis-yolo_amd", "**", "*.py"), recursive=True):
        names |= _python_names(_read(path))
    for path in glob.glob(os.path.join(ROOT, "dis-yolo_amd", "csrc", "**", "*"), recursive=True):
        if os.path.isfile(path) and path.endswith((".hip", ".h", ".cpp", ".hpp")):
            names |= set(C_NAME.findall(C_COMMENT.sub(" ", _read(path))))
    return names


def _design_names():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    section = text.split("## 7b. Environment switches", 1)[1].split("\n## ", 1)[0]
    rows = [ln for ln in section.splitlines() if ln.startswith("| `DISYOLO_")]
    return [re.match(r"\| `" + NAME + "`", ln).group(1) for ln in rows]


def test_design_table_lists_exactly_the_switches_the_code_reads():
    table = _design_names()
    assert len(table) == len(set(table)), "a switch is listed twice in DESIGN.md"
    src = _source_names()
    assert src, "the scan found no switch at all: the patterns no longer match the source"
    assert src == set(table), "read but not in DESIGN.md: %s; in DESIGN.md but not read: %s" % (
        sorted(src - set(table)), sorted(set(table) - src))


def test_bench_reads_only_listed_switches():
    names = _python_names(_read(os.path.join(ROOT, "bench.py")))
    assert names, "bench.py is expected to read DISYOLO_SIDE_LANE"
    assert names <= set(_design_names()), "bench.py reads %s, not in DESIGN.md" % sorted(names - set(_design_names()))
