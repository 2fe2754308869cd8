"""CPU: INTEGRATION.md's switch table names exactly the NBM_* environment variables that the package reads."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'birdsoundclassif_amd')


def read_switches():
    """NBM_* names read through os.environ.get(...) / os.environ[...] / getenv(...) in Python and getenv("...") in csrc."""
    names = {}
    py = re.compile(r'''(?:environ\.get|environ\[|getenv)\(?\s*['"](NBM_[A-Z0-9_]+)['"]''')
    c = re.compile(r'''\bgetenv\(\s*"(NBM_[A-Z0-9_]+)"''')
    files = [(f, py) for f in glob.glob(os.path.join(PKG, '**', '*.py'), recursive=True)]
    files += [(f, c) for f in glob.glob(os.path.join(PKG, 'csrc', '*')) if os.path.isfile(f) and not f.endswith(('.o', '.so'))]
    for f, rx in files:
        for n in rx.findall(open(f, errors='replace').read()):
            names.setdefault(n, set()).add(os.path.relpath(f, ROOT))
    return names


def documented_switches():
    """NBM_* names in the first column of the `| switch | ... |` table of INTEGRATION.md."""
    lines = open(os.path.join(ROOT, 'INTEGRATION.md')).read().splitlines()
    start = [i for i, l in enumerate(lines) if re.match(r'\|\s*switch\s*\|', l)]
    assert len(start) == 1, 'INTEGRATION.md must hold exactly one switch table'
    names = set()
    for l in lines[start[0] + 2:]:
        if not l.startswith('|'):
            break
        names |= set(re.findall(r'NBM_[A-Z0-9_]+', l.split('|')[1]))
    return names


def test_switch_table_lists_exactly_the_switches_the_package_reads():
    read, doc = read_switches(), documented_switches()
    assert 'NBM_SPLIT_BF16' in read and 'NBM_LIB' in read          # the scan sees both the C library and the Python side
    missing = {n: sorted(f) for n, f in read.items() if n not in doc}
    stale = sorted(doc - set(read))
    assert not missing, f'read by the package but not in INTEGRATION.md\'s switch table: {missing}'
    assert not stale, f'in INTEGRATION.md\'s switch table but read nowhere: {stale}'
