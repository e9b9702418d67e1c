"""The runtime-knob table of INTEGRATION.md §7 and the code agree: every
environment variable the native sources read is listed, and every variable
listed is read somewhere.  Reads files only."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'optimalinterpolation_amd', 'csrc')


def _read(path):
    with open(path, encoding='utf-8') as f:
        return f.read()


def _section7():
    text = _read(os.path.join(ROOT, 'INTEGRATION.md'))
    start = text.index('\n## 7.')
    end = text.find('\n## ', start + 1)
    return text[start:end if end >= 0 else len(text)]


def _csrc_reads():
    """OI_* names passed to getenv (or the engine's env_int) in csrc/."""
    names = set()
    for path in sorted(glob.glob(os.path.join(CSRC, '*'))):
        names.update(re.findall(r'\b(?:getenv|env_int)\(\s*"(OI_[A-Z0-9_]+)"', _read(path)))
    return names


def test_every_knob_read_is_documented():
    section = _section7()
    reads = _csrc_reads()
    assert len(reads) >= 10, reads  # the search itself still finds the knobs
    missing = sorted(n for n in reads if not re.search(r'\b%s\b' % n, section))
    assert not missing, missing


def test_every_documented_knob_is_read():
    rows = [l for l in _section7().splitlines() if l.startswith('|')]
    listed = set()
    for row in rows:
        first = row.split('|')[1]
        listed.update(re.findall(r'`(OI_[A-Z0-9_]+)', first))
    assert len(listed) >= 10, listed
    sources = sorted(glob.glob(os.path.join(CSRC, '*')))
    sources += sorted(glob.glob(os.path.join(ROOT, 'optimalinterpolation_amd', '*.py')))
    sources.append(os.path.join(ROOT, 'bench.py'))
    quoted = set()
    for path in sources:
        quoted.update(re.findall(r'''["'](OI_[A-Z0-9_]+)["']''', _read(path)))
    unread = sorted(listed - quoted)
    assert not unread, unread
