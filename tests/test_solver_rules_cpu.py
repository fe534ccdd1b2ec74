"""The decisions of the rank-1 solve (when the squarings stop, which result is suspect, the eigenvalue clamp) are stated once, in
k_solve.h: outside comments and #define / #ifndef lines their constants occur in no other file of disco_amd/csrc.  A fifth solver
uses the rules of k_solve.h; it does not write them out again."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'disco_amd', 'csrc')
NAMES = ('DISCO_SQUARING_DONE', 'DISCO_KEPT_TAU_MIN', 'SOLVE_ETA', '1.7e308')


def _code(text):
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lines = [re.sub(r'//.*', '', ln) for ln in text.split('\n')]
    return '\n'.join(ln for ln in lines if not re.match(r'\s*#\s*(define|ifndef)\b', ln))


def test_solver_rules_are_stated_in_k_solve_h_only():
    elsewhere = []
    for f in sorted(os.listdir(CSRC)):
        code = _code(open(os.path.join(CSRC, f)).read())
        elsewhere += [(f, name) for name in NAMES if name in code and f != 'k_solve.h']
    assert not elsewhere, elsewhere
    stated = open(os.path.join(CSRC, 'k_solve.h')).read()
    assert all(name in stated for name in NAMES)
