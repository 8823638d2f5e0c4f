"""fgvc_amd/build.py decides what is stale from build.HEADERS: every file that a source under fgvc_amd/csrc/ includes by name must be in it,
or a regenerated schedule (tools/gen_*.py) or an edited header relinks the old objects without a word."""
import os
import re

from fgvc_amd import build


def test_every_quoted_include_is_a_build_dependency():
    headers = {os.path.realpath(h) for h in build.HEADERS}
    assert all(os.path.isfile(h) for h in headers)
    seen = 0
    for name in sorted(os.listdir(build.CSRC)):
        path = os.path.join(build.CSRC, name)
        with open(path) as fh:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M):
                seen += 1
                assert os.path.realpath(os.path.join(build.CSRC, inc)) in headers, f"{name} includes {inc}: not in build.HEADERS"
    assert seen > 20                                                              # the pattern still finds the includes
