"""Helpers live in one place: no top-level helper function of three or more body lines may be
byte-identical in two test modules.  Shared ones belong in checkers.py, gpu_support.py, abi_surface.py,
isa_tools.py or the family's own helper module."""
import ast
from pathlib import Path

TESTS = Path(__file__).resolve().parent


def test_no_helper_is_copied_between_modules():
    seen, copies = {}, []
    for path in sorted(TESTS.glob("*.py")):
        text = path.read_text()
        for node in ast.parse(text).body:
            if not isinstance(node, (ast.FunctionDef, ast.AsyncFunctionDef)) or node.name.startswith("test_"):
                continue
            if node.end_lineno - node.body[0].lineno + 1 < 3:
                continue
            src = ast.get_source_segment(text, node)
            first = seen.setdefault(src, path.name)
            if first != path.name:
                copies.append(f"{node.name}: {first} and {path.name}")
    assert not copies, "copied helpers (move each to a shared module):\n  " + "\n  ".join(copies)
