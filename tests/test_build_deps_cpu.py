"""Every file a native target's sources include is named in that target's build recipe.

_build.build() rebuilds a library when one of its `srcs` or `deps` is newer than it; a header that is included but not
listed could be edited and the old library would go on being used.  Text only: the `#include "..."` lines are followed
transitively from the sources, resolved against the including file's directory, csrc/ and include/."""
import os
import re

import pytest

from libmultirobotplanning_amd import _build

_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def _resolve(name, includer):
    for base in (os.path.dirname(includer), _build.CSRC, _build.INCLUDE):
        p = os.path.normpath(os.path.join(base, name))
        if os.path.isfile(p):
            return p
    raise AssertionError('%s includes "%s", which is neither next to it nor under csrc/ or include/' % (includer, name))


def _closure(srcs):
    seen, todo = set(), list(srcs)
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        with open(f) as fh:
            todo.extend(_resolve(name, f) for name in _INCLUDE.findall(fh.read()))
    return seen


@pytest.mark.parametrize("target", sorted(_build.TARGETS))
def test_every_included_file_is_a_listed_dependency(target):
    spec = _build.TARGETS[target]
    srcs = [os.path.normpath(os.path.join(_build.CSRC, s)) for s in spec["srcs"]]
    listed = set(srcs) | {os.path.normpath(os.path.join(_build.CSRC, d)) for d in spec["deps"]}
    missing = sorted(os.path.relpath(f, _build.CSRC) for f in _closure(srcs) - listed)
    assert not missing, "%s: included but not in srcs/deps of _build.TARGETS: %s" % (target, missing)
