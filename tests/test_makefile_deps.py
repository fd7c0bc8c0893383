"""csrc/Makefile rebuilds one object per translation unit, so its prerequisite lists decide whether a build after an edit is
correct: every project header a unit reaches through #include "..." must be a prerequisite of its object, and HDRS (the
profiling and A/B builds compile every source at once) must hold them all.  No GPU, no compiler, no make: the Makefile's
text with its variables expanded, the sources' include lines by regular expression."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myrrix-recommender_amd", "csrc")
INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)
ASSIGN = re.compile(r"^([A-Za-z_][A-Za-z0-9_]*)[ \t]*[?:]?=[ \t]*(.*)$")
RULE = re.compile(r"^([^\t#=:][^=:]*):(?!=)(.*)$")


def _makefile():
    """-> (variables, {target: [prerequisites]}), every $(NAME) expanded"""
    variables, rules = {}, {}
    with open(os.path.join(CSRC, "Makefile")) as f:
        lines = f.read().replace("\\\n", " ").split("\n")

    def expand(text):
        for _ in range(20):
            new = re.sub(r"\$\((\w+)\)", lambda m: variables.get(m.group(1), ""), text)
            if new == text:
                return text
            text = new
        raise AssertionError("variable loop in the Makefile: " + text)

    for line in lines:
        m = ASSIGN.match(line)
        if m:
            variables[m.group(1)] = m.group(2)
            continue
        m = RULE.match(line)
        if m:
            for target in expand(m.group(1)).split():
                rules.setdefault(target, []).extend(expand(m.group(2)).split())
    return {k: expand(v) for k, v in variables.items()}, rules


def _norm(path, base=CSRC):
    return os.path.normpath(os.path.relpath(os.path.join(base, path), CSRC))


def _reachable_headers(source):
    """project headers reachable from csrc/<source>, as paths relative to csrc/"""
    seen, todo = set(), [_norm(source)]
    while todo:
        cur = todo.pop()
        with open(os.path.join(CSRC, cur)) as f:
            text = f.read()
        for inc in INCLUDE.findall(text):
            h = _norm(inc, os.path.dirname(os.path.join(CSRC, cur)))
            assert os.path.isfile(os.path.join(CSRC, h)), "%s includes \"%s\", which is not in the tree" % (cur, inc)
            if h not in seen:
                seen.add(h)
                todo.append(h)
    return seen


def _objects():
    variables, rules = _makefile()
    objects = {}
    for target, prereqs in rules.items():
        if target.endswith(".o"):
            sources = [p for p in prereqs if p.endswith((".hip", ".cpp"))]
            assert len(sources) == 1, (target, prereqs)
            objects[target] = (sources[0], {_norm(p) for p in prereqs})
    return variables, objects


def test_every_source_has_an_object():
    variables, objects = _objects()
    assert sorted(src for src, _ in objects.values()) == sorted(variables["SRCS"].split())


def test_every_reachable_header_is_a_prerequisite_of_its_object():
    _, objects = _objects()
    missing = {}
    for target, (source, prereqs) in sorted(objects.items()):
        lacking = sorted(_reachable_headers(source) - prereqs)
        if lacking:
            missing[target] = lacking
    assert not missing, "headers a unit includes but its object does not depend on: %r" % missing


def test_hdrs_holds_every_reachable_header():
    variables, objects = _objects()
    hdrs = {_norm(p) for p in variables["HDRS"].split()}
    reachable = set()
    for source, _ in objects.values():
        reachable |= _reachable_headers(source)
    assert not sorted(reachable - hdrs), "headers missing from HDRS: %r" % sorted(reachable - hdrs)
