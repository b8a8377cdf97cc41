"""tools/variants.py stays in step with the kernels: no variant is defined twice, every macro a variant sets is
a switch some source under csrc/ reads (`#ifndef IBL_X`), and the side tables name existing variants. The file
is parsed, not imported (importing it loads the build module)."""
import ast
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "informationbottleneckdecodingldpc_amd", "csrc")


def _tables():
    tree = ast.parse(open(os.path.join(ROOT, "tools", "variants.py")).read())
    out = {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and isinstance(node.value, ast.Dict):
            out[node.targets[0].id] = node.value
    return out


def _keys(d):
    return [ast.literal_eval(k) for k in d.keys]   # a dict display keeps repeated keys; the built dict would not


def test_no_variant_is_defined_twice():
    keys = _keys(_tables()["VARIANTS"])
    assert keys, "VARIANTS not found"
    twice = sorted({k for k in keys if keys.count(k) > 1})
    assert not twice, f"variants defined more than once: {twice}"


def test_every_variant_macro_is_read_by_the_sources():
    known = set()
    for f in os.listdir(CSRC):
        if f.endswith((".hip", ".h", ".inc")):
            known |= set(re.findall(r"^\s*#\s*ifndef\s+(IBL_\w+)", open(os.path.join(CSRC, f)).read(), re.M))
    variants = _tables()["VARIANTS"]
    stale = []
    for name, defines in zip(_keys(variants), variants.values):
        for d in ast.literal_eval(defines):
            macro = d.split("=", 1)[0]
            assert macro.startswith("IBL_"), (name, d)
            if macro not in known:
                stale.append((name, macro))
    assert not stale, f"variants that set a macro no source reads: {stale}"


def test_side_tables_name_existing_variants():
    t = _tables()
    names = set(_keys(t["VARIANTS"]))
    for table in ("SCHED_ARGS", "SRC_FLAGS"):
        missing = sorted(set(_keys(t[table])) - names)
        assert not missing, f"{table} names unknown variants: {missing}"
