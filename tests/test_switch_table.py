"""DESIGN.md §3.4 lists every MTLSSL_* environment variable the product reads, and nothing else; the names it lists as
retired occur nowhere in the package. A new switch therefore needs a row (default, effect, what flips it), and a
retired one cannot come back unseen."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = re.compile(r"MTLSSL_[A-Z0-9_]+")
MAX_SWITCHES = 34


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _product_files():
    pkg = os.path.join(ROOT, "mtl_ssl_amd")
    files = glob.glob(os.path.join(pkg, "**", "*.py"), recursive=True)
    files += [p for p in glob.glob(os.path.join(pkg, "csrc", "*")) if os.path.isfile(p)]
    return files + [os.path.join(ROOT, "bench.py")]


def _names_read():
    """Every MTLSSL_* token on a line that reads the environment."""
    names = set()
    for path in _product_files():
        for line in _read(path).splitlines():
            if "environ" in line or "getenv" in line:
                names.update(NAME.findall(line))
    return names


def _section_tables():
    """(names in the first column of the switch table, names in the first column of the retired table) of §3.4."""
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("### 3.4 ")
    section = text[start:text.index("\n### ", start + 1)]
    live, retired = section.split("**Retired switches.**")

    def first_column(part):
        return {n for line in part.splitlines() if line.startswith("| `MTLSSL_") for n in NAME.findall(line.split("|")[1])}

    return first_column(live), first_column(retired)


def test_design_table_lists_exactly_the_switches_the_product_reads():
    read = _names_read()
    live, retired = _section_tables()
    assert read == live, "read but not in DESIGN.md §3.4: %s; listed but not read: %s" % (
        sorted(read - live), sorted(live - read))
    assert len(read) <= MAX_SWITCHES, sorted(read)
    assert len(retired) == 25 and not (retired & live), sorted(retired & live)


def test_retired_switches_are_gone_from_the_package():
    _, retired = _section_tables()
    assert retired
    hits = []
    for path in glob.glob(os.path.join(ROOT, "mtl_ssl_amd", "**", "*"), recursive=True):
        if os.path.isfile(path) and not path.endswith((".so", ".o", ".pyc", ".a")):
            found = set(NAME.findall(_read(path))) & retired
            if found:
                hits.append((os.path.relpath(path, ROOT), sorted(found)))
    assert not hits, hits
