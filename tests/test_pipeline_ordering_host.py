"""Every entry point that takes a context is ordered behind the frames submitted before it (include/dogeray_amd.h, dr_pipeline_submit): a source
check, in the spirit of test_library_exports_every_declared_symbol.  An extern "C" function of dogeray_amd/csrc/context*.cpp whose first parameter
is a dr_context* must call join_pipeline( or pipeline_flush( in its body, or call a function of the same file that does, or stand in EXEMPT below
with its reason -- so a later entry point cannot leave the pipeline out without saying why."""
import glob
import os
import re

from conftest import ROOT

CSRC = os.path.join(ROOT, "dogeray_amd", "csrc")

# entry points that need no ordering against held frames: name (or prefix*) -> why
EXEMPT = {
    "dr_pipeline_*": "the pipeline itself: submit holds frames, wait and image launch the group of the ticket they are asked for",
    "dr_context_destroy": "the destructor drains every stream; frames still held are dropped with the context",
    "dr_context_stream": "hands out the stream handle, touches no device state",
    "dr_context_get_option": "reads host members; takes a const context",
}

DEFINITION = re.compile(r"^(?:static\s+|inline\s+)*[A-Za-z_][\w:<>\s\*&]*?\b([A-Za-z_]\w*)\((.*)$")
JOINS = re.compile(r"\b(?:join_pipeline|pipeline_flush)\(")


def functions(text):
    """[(name, rest of the signature line, body, inside extern "C")] of the definitions that start in column 0; a body runs to the closing brace in
    column 0 (a definition written on one line is its own body)"""
    out, lines, in_c, k = [], text.split("\n"), False, 0
    while k < len(lines):
        line = lines[k]
        if line.startswith('extern "C" {'):
            in_c = True
        elif line.startswith("}") and "extern" in line:
            in_c = False
        m = DEFINITION.match(line)
        if m and not line.startswith(("#", "//", "}", "using ", "namespace ", "typedef ", "struct ", "constexpr ", "const Option")):
            sig_end = k
            while "{" not in lines[sig_end] and not lines[sig_end].rstrip().endswith(";"):
                sig_end += 1
            if "{" in lines[sig_end]:
                if lines[sig_end].rstrip().endswith("}"):
                    end = sig_end
                else:
                    end = next(j for j in range(sig_end + 1, len(lines)) if lines[j].startswith("}"))
                body = "\n".join(lines[k:end + 1])
                body = re.sub(r"//[^\n]*", "", re.sub(r'"(?:\\.|[^"\\\n])*"', '""', body))      # a name in a message or a comment is no call
                out.append((m.group(1), " ".join(lines[k:sig_end + 1]), body, in_c))
                k = end
        k += 1
    return out


def entry_point(name, sig, in_c):
    """an exported function (inside extern "C", not static) whose first parameter is a context"""
    return in_c and not sig.startswith("static") and re.search(r"\b%s\(\s*(?:const\s+)?dr_context\s*\*" % re.escape(name), sig) is not None


def unordered_entry_points(text):
    """names of the extern "C" functions with a dr_context* first that neither join the pipeline, nor call a function of this file that does, nor are
    exempt; and the names of those that are exempt"""
    fns = functions(text)
    joins = {name for name, _, body, _ in fns if JOINS.search(body)}
    grew = True
    while grew:          # a function that calls one that joins, joins
        grew = False
        for name, _, body, _ in fns:
            if name not in joins and any(re.search(r"\b%s\(" % re.escape(j), body.split("\n", 1)[-1] if "\n" in body else "") for j in joins):
                joins.add(name)
                grew = True
    bad, exempt = [], []
    for name, sig, _, in_c in fns:
        if not entry_point(name, sig, in_c):
            continue
        if name in joins:
            continue
        if any(name == e or (e.endswith("*") and name.startswith(e[:-1])) for e in EXEMPT):
            exempt.append(name)
        else:
            bad.append(name)
    return bad, exempt


def test_every_context_entry_point_is_ordered_behind_the_pipeline():
    files = sorted(glob.glob(os.path.join(CSRC, "context*.cpp")))
    assert len(files) >= 6
    seen, exempt_seen = [], []
    for path in files:
        with open(path) as f:
            text = f.read()
        seen += [name for name, sig, _, in_c in functions(text) if entry_point(name, sig, in_c)]
        bad, exempt = unordered_entry_points(text)
        exempt_seen += exempt
        assert not bad, "%s: %s neither call join_pipeline / pipeline_flush (nor a function of the file that does) nor stand in EXEMPT" % (os.path.basename(path), ", ".join(bad))
    # the parser found what the header declares: every declared function with a context first is one of them
    with open(os.path.join(ROOT, "include", "dogeray_amd.h")) as f:
        declared = set(re.findall(r"^\w[\w\s\*]*?\b(dr_\w+)\(\s*(?:const\s+)?dr_context\s*\*", f.read(), re.M))
    assert len(declared) >= 50 and declared <= set(seen), "not found in context*.cpp: %s" % ", ".join(sorted(declared - set(seen)))
    # and the table holds nothing stale
    for e in EXEMPT:
        assert any(n == e or (e.endswith("*") and n.startswith(e[:-1])) for n in exempt_seen), "EXEMPT names %s, which is no unordered entry point" % e


def test_the_check_catches_an_entry_point_that_forgets_the_pipeline():
    """the parser on a file made for it: a direct call, a call through a helper, a one-line definition, an exempt name and the omission"""
    text = "\n".join([
        "namespace {",
        "int helper(dr_context* c) {",
        "  return join_pipeline(c);",
        "}",
        "int other(dr_context* c) { return 0; }",
        "}  // namespace",
        'extern "C" {',
        "int dr_direct(dr_context* c) {",
        "  DR_TRY(pipeline_flush(c));",
        "  return DR_OK;",
        "}",
        "int dr_through(dr_context* c, int x,",
        "               int y) {",
        "  return helper(c);",
        "}",
        "int dr_forgets(dr_context* c) {",
        "  if (c) { other(c); }      // join_pipeline(c) is missing",
        '  set_error("helper(c) comes first");',
        "  return DR_OK;",
        "}",
        "void dr_context_destroy(dr_context* c) { delete c; }",
        "int dr_no_context(int n) { return n; }",
        "static int not_exported(dr_context* c) { return 0; }",
        '}  // extern "C"',
        "int dr_outside(dr_context* c) { return 0; }",
    ])
    assert [f[0] for f in functions(text)] == ["helper", "other", "dr_direct", "dr_through", "dr_forgets", "dr_context_destroy", "dr_no_context", "not_exported", "dr_outside"]
    assert unordered_entry_points(text) == (["dr_forgets"], ["dr_context_destroy"])
