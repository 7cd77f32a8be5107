"""How csrc/Makefile knows which headers an object depends on, for the tests that hold a header to be a prerequisite of
the objects that include it: the object rule has the compiler write every object's real prerequisites beside it
(-MMD -MP) and the Makefile includes those lists, so a touched header rebuilds exactly its includers."""
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'metalens_amd', 'csrc')


def header_is_prerequisite(header, unit):
    """`header` (e.g. 'fields_pupil.h') is a prerequisite of `unit`.o (e.g. 'fields_pupil'): the unit is one of SRCS, the
    object rule generates dependencies and they are included; the unit includes the header; and where the build has
    written the unit's list, the list names the header."""
    made = open(os.path.join(CSRC, 'Makefile')).read()
    rule = re.search(r'^\$\(BUILD\)/%\.o: %\.hip\n(?:\t.*\n)*?\t\$\(HIPCC\) .*-MMD -MP .*-c \$< -o \$@$', made, re.M)
    if not rule or not re.search(r'^-include \$\(OBJS:\.o=\.d\)$', made, re.M):
        return False
    if not re.search(r'^SRCS\s*:=.*\b%s\.hip\b' % re.escape(unit), made, re.M):
        return False
    if not _includes(os.path.join(CSRC, unit + '.hip'), header, set()):
        return False
    listed = os.path.join(CSRC, 'build', unit + '.d')
    return not os.path.exists(listed) or header in re.split(r'[\s\\:]+', open(listed).read())


def _includes(path, header, seen):
    """`path` includes `header`, itself or through the project's own headers"""
    for name in re.findall(r'^#include "([^"]+)"', open(path).read(), re.M):
        if name == header:
            return True
        nested = os.path.join(CSRC, name)
        if name not in seen and os.path.exists(nested):
            seen.add(name)
            if _includes(nested, header, seen):
                return True
    return False
