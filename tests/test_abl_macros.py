"""Every macro csrc/build_abl.sh defines must still switch something: each
-DNAME of the script has to occur in the code of a source file under csrc/
outside the macro's own default block (`#ifndef NAME` / `#define NAME ...` /
`#endif`).  Comments do not count.  A variant whose macro no code reads builds
the default library under another name.
"""
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "victoriametrics_amd", "csrc")


def _macros():
    with open(os.path.join(CSRC, "build_abl.sh")) as f:
        lines = [ln for ln in f if not ln.lstrip().startswith("#")]
    return sorted(set(re.findall(r"-D(\w+)", "".join(lines))))


def _code():
    """All .hip/.h text under csrc/ with the comments taken out."""
    out = []
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")):
            with open(os.path.join(CSRC, name)) as f:
                out.append(f.read())
    text = "\n".join(out)
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", " ", text)


def test_every_abl_macro_is_read():
    macros = _macros()
    assert macros, "build_abl.sh defines no macro"
    code = _code()
    unread = []
    for m in macros:
        name = re.escape(m)
        rest = re.sub(r"#\s*ifndef\s+%s\s*\n\s*#\s*define\s+%s\b[^\n]*\n\s*#\s*endif"
                      % (name, name), " ", code)
        if not re.search(r"\b%s\b" % name, rest):
            unread.append(m)
    assert not unread, "build_abl.sh defines macros no code reads: %s" % unread
