"""The development switches the library reads (CLRSDP_* names passed to env_on / env_off / env_int
in clrsdp.hip) and the table of them in DESIGN.md section 13 are the same set, and the library
reads its environment through those three helpers only."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "clustered-low-rank-sdp-solver_amd", "csrc", "clrsdp.hip")


def _library_switches():
    src = open(SRC, encoding="utf-8").read()
    return src, set(re.findall(r'\benv_(?:on|off|int)\(\s*"(CLRSDP_[A-Z0-9_]+)"', src))


def _design_table():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    section = text.split("## 13. Development switches", 1)[1].split("**Retired**", 1)[0]
    return set(re.findall(r"^\| `(CLRSDP_[A-Z0-9_]+)` \|", section, flags=re.M))


def test_design_switch_table_matches_library():
    src, read = _library_switches()
    table = _design_table()
    # the three helpers' own reads take the name as a parameter; nothing names a switch to getenv
    assert len(re.findall(r"\bgetenv\(", src)) == 3
    assert not re.findall(r'getenv\(\s*"', src)
    assert len(read) > 10, read
    assert read == table, {"only in clrsdp.hip": sorted(read - table),
                           "only in DESIGN.md": sorted(table - read)}

