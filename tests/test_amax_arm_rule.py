"""An armed magnitude-slot pointer never outlives its call (CPU).

m3t_amax_out parks a pointer in a thread-local that the NEXT producing library call takes.  A call that raises before the C side runs
(ctypes refusing an argument) would leave it parked for an unrelated later kernel, so m3t/ops.py arms in one place only: _armed_call,
which clears the pointer on any failure.  This rule keeps every other arm site out of that file."""
import ast
import os

from conftest import PKG

OPS = os.path.join(PKG, "m3t", "ops.py")


def _violations(source):
    """(line, what) for every reference to the attribute m3t_amax_out outside amax_out / _amax_clear and every call of amax_out or
    _amax_clear outside _armed_call"""
    bad = []

    def walk(node, owner):
        for child in ast.iter_child_nodes(node):
            inside = child.name if isinstance(child, (ast.FunctionDef, ast.AsyncFunctionDef)) and owner is None else owner
            if isinstance(child, ast.Attribute) and child.attr == "m3t_amax_out" and owner not in ("amax_out", "_amax_clear"):
                bad.append((child.lineno, "m3t_amax_out in %s" % (owner or "<module>")))
            if isinstance(child, ast.Call) and owner != "_armed_call":
                f = child.func
                name = f.id if isinstance(f, ast.Name) else f.attr if isinstance(f, ast.Attribute) else None
                if name in ("amax_out", "_amax_clear"):
                    bad.append((child.lineno, "%s() in %s" % (name, owner or "<module>")))
            walk(child, inside)

    walk(ast.parse(source), None)
    return bad


def test_the_rule_catches_a_bare_arm():
    assert _violations("def f(p):\n    amax_out(p)\n    lib().m3t_x()\n") == [(2, "amax_out() in f")]
    assert _violations("class A:\n    def g(self):\n        try:\n            ops.amax_out(1)\n        except E:\n            _amax_clear()\n") \
        == [(4, "amax_out() in g"), (6, "_amax_clear() in g")]
    assert _violations("def h():\n    lib().m3t_amax_out(None)\n") == [(2, "m3t_amax_out in h")]
    assert not _violations("def amax_out(s):\n    lib().m3t_amax_out(s)\n\ndef _armed_call(s, e, *a):\n    amax_out(s)\n    _amax_clear()\n")


def test_ops_arms_only_in_armed_call():
    with open(OPS) as fh:
        source = fh.read()
    names = {n.name for n in ast.parse(source).body if isinstance(n, ast.FunctionDef)}
    assert {"amax_out", "_amax_clear", "_armed_call"} <= names, "m3t/ops.py no longer defines the three functions this rule is about"
    bad = _violations(source)
    assert not bad, "arm through _armed_call (an armed pointer must not outlive its call):\n" + "\n".join("ops.py:%d: %s" % b for b in bad)
