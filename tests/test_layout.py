"""Where the code lives: the references are importable modules under oracle/, which stand on their own, and no test module is
another test module's library.  Two walks over the imports of the sources, nothing run."""
import ast
import glob
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def imported_modules(path):
    """(line, dotted module name) of every import statement of the file, at any depth; `from . import x` gives '.'"""
    out = []
    for node in ast.walk(ast.parse(open(path).read(), path)):
        if isinstance(node, ast.Import):
            out += [(node.lineno, a.name) for a in node.names]
        elif isinstance(node, ast.ImportFrom):
            out.append((node.lineno, "." * node.level + (node.module or "")))
    return out


def sources(folder):
    files = sorted(glob.glob(os.path.join(ROOT, folder, "**", "*.py"), recursive=True))
    assert files, folder
    return files


def test_no_test_module_is_imported_by_another():
    bad = [(os.path.relpath(f, ROOT), line, mod) for f in sources("tests") for line, mod in imported_modules(f)
           if any(part.startswith("test_") for part in mod.split("."))]
    assert bad == []


def test_the_oracle_imports_neither_the_product_nor_its_tests_and_tools():
    bad = [(os.path.relpath(f, ROOT), line, mod) for f in sources("oracle") for line, mod in imported_modules(f)
           if mod.split(".")[0] in ("reef_amd", "tests", "tools")]
    assert bad == []
