"""The development switches the library reads (CLRSDP_* names passed to env_on / env_off / env_int
in clrsdp.hip) and the table of them in DESIGN.md section 13 are the same set, the library
reads its environment through those three helpers only, and every such read stands in
Switches::read, each name once."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "clustered-low-rank-sdp-solver_amd", "csrc", "clrsdp.hip")
CALL = r"\benv_(?:on|off|int)\("


def _library_switches():
    src = open(SRC, encoding="utf-8").read()
    return src, set(re.findall(CALL + r'\s*"(CLRSDP_[A-Z0-9_]+)"', src))


def _design_table():
    text = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    section = text.split("## 13. Development switches", 1)[1].split("**Retired**", 1)[0]
    return set(re.findall(r"^\| `(CLRSDP_[A-Z0-9_]+)` \|", section, flags=re.M))


def _read_body(src):
    """(start, end) of the body of Switches::read: from its opening brace to the matching one."""
    start = src.index("static Switches read() {")
    depth, pos = 0, src.index("{", start)
    for end in range(pos, len(src)):
        depth += {"{": 1, "}": -1}.get(src[end], 0)
        if depth == 0:
            return pos, end
    raise AssertionError("Switches::read: no closing brace")


def test_design_switch_table_matches_library():
    src, read = _library_switches()
    table = _design_table()
    # the three helpers' own reads take the name as a parameter; nothing names a switch to getenv
    assert len(re.findall(r"\bgetenv\(", src)) == 3
    assert not re.findall(r'getenv\(\s*"', src)
    assert len(read) > 10, read
    assert read == table, {"only in clrsdp.hip": sorted(read - table),
                           "only in DESIGN.md": sorted(table - read)}


def test_every_switch_is_read_once_in_switches_read():
    src, read = _library_switches()
    lo, hi = _read_body(src)
    calls = [m.start() for m in re.finditer(CALL, src)]
    # the three definitions (`bool env_on(const char* name ...`) are the only calls' look-alikes
    # outside read(); every other one lies inside it
    defs = [m.start(1) for m in
            re.finditer(r"static inline (?:bool|long) (env_(?:on|off|int)\()const char\* name", src)]
    assert len(defs) == 3
    outside = [p for p in calls if not lo < p < hi and p not in defs]
    assert not outside, [src[p:p + 60] for p in outside]
    # each name is read at exactly one place, and stands nowhere else as a string of its own
    for name in sorted(read):
        assert len(re.findall(CALL + r'\s*"%s"' % name, src)) == 1, name
        assert src.count('"%s"' % name) == 1, name
    # nothing caches a switch in a static, and the plans do not reach for the environment
    assert not re.findall(r"static\s+const\s+\w+\s+\w+\s*=\s*!?env_", src)
    for gone in ("la_opts()", "trsm_blk_mode", "lu_blk_mode", "chain_on", "mxblk_on",
                 "takes_potrf_batched"):
        assert gone not in src, gone
