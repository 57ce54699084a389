"""CPU check of tests/kernel_forms.py against the C ABI's option setter (csrc/api.hip: gpsig_set_option) and the context's initialisers
(csrc/ctx.hpp): every option is registered, every registered test exists, every recorded default is the real one."""
import ast
import os
import re

import pytest

import kernel_forms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gpsig_amd", "csrc")
TESTS = os.path.join(ROOT, "tests")


def setter_options(src):
    """option name -> the gpsig_ctx field its branch assigns, from the strcmp chain of gpsig_set_option."""
    body = src[src.index("int gpsig_set_option("):]
    body = body[:body.index("\n}\n")]
    out = {}
    for line in body.splitlines():
        m = re.search(r'strcmp\(name, "([^"]*)"\)\)(.*)', line)
        if m:
            f = re.search(r"c->(\w+)\s*=", m.group(2))
            out[m.group(1)] = f.group(1) if f else None
    return out


def ctx_defaults(src):
    """field -> integer initialiser of the plain int members of struct gpsig_ctx."""
    body = src[src.index("struct gpsig_ctx {"):]
    body = body[:body.index("\n};")]
    out = {}
    for line in body.splitlines():
        code = line.split("//")[0].strip()
        if not code.startswith("int "):
            continue
        for name, value in re.findall(r"(\w+)\s*=\s*(-?\d+)", code):
            out[name] = int(value)
    return out


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_every_option_of_the_setter_is_registered():
    opts = setter_options(_read(CSRC, "api.hip"))
    assert len(opts) >= 40, "the strcmp chain of gpsig_set_option was not found where expected"
    assert set(opts) == set(kernel_forms.OPTIONS), ("options without an entry", sorted(set(opts) - set(kernel_forms.OPTIONS)),
                                                    "entries without an option", sorted(set(kernel_forms.OPTIONS) - set(opts)))


def test_the_parser_notices_a_new_option():
    src = _read(CSRC, "api.hip")
    fake = src.replace('if (!strcmp(name, "glds"))', 'if (!strcmp(name, "x")) c->x = value;\n    else if (!strcmp(name, "glds"))', 1)
    assert "x" in setter_options(fake) and "x" not in kernel_forms.OPTIONS


@pytest.mark.parametrize("name", sorted(kernel_forms.OPTIONS))
def test_entry_is_well_formed_and_its_tests_exist(name):
    e = kernel_forms.OPTIONS[name]
    assert isinstance(e.get("default"), int), name
    if "exempt" in e:
        assert set(e) == {"default", "exempt"} and isinstance(e["exempt"], str) and e["exempt"].strip() and "\n" not in e["exempt"], name
        return
    assert set(e) == {"default", "values", "tests"}, name
    assert e["values"] and all(isinstance(v, int) for v in e["values"]), name
    assert e["tests"], name
    for node in e["tests"]:
        fname, _, func = node.partition("::")
        path = os.path.join(TESTS, fname)
        assert os.path.isfile(path), (name, node)
        tree = ast.parse(_read(path))
        funcs = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
        assert func.startswith("test_") and func in funcs, (name, node)


def test_recorded_defaults_are_the_context_initialisers():
    opts = setter_options(_read(CSRC, "api.hip"))
    init = ctx_defaults(_read(CSRC, "ctx.hpp"))
    for name, field in sorted(opts.items()):
        assert field in init, (name, field, "no integer initialiser in struct gpsig_ctx")
        assert kernel_forms.OPTIONS[name]["default"] == init[field], (name, field, kernel_forms.OPTIONS[name]["default"], init[field])
