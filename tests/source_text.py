"""The text a library is compiled from, for the CPU tests that assert over source text: a .hip and the headers of lle_amd/ it
includes, directly or through another of them.  The public C headers (include/*.h) declare the ABI and are not part of it."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def files_of(hip):
    """Paths relative to the repository root: `hip` first, then every "..."-included file under lle_amd/ in the order found."""
    found, todo = [], [os.path.normpath(hip)]
    while todo:
        path = todo.pop(0)
        if path in found:
            continue
        found.append(path)
        for inc in re.findall(r'^#include "([^"]+)"', open(os.path.join(ROOT, path)).read(), re.M):
            target = os.path.normpath(os.path.join(os.path.dirname(path), inc))
            if target.startswith("lle_amd" + os.sep):
                todo.append(target)
    return found


def text_of(hip):
    return "".join(open(os.path.join(ROOT, p)).read() for p in files_of(hip))


def update_path_of(hip, update_function):
    """What an lle_*_update call runs that is not the launch: the .hip from `update_function` on, and the shared core from its
    checks on (lle_amd/coop/tracker_core.hpp: check_update_args, update)."""
    source = open(os.path.join(ROOT, hip)).read()
    core = open(os.path.join(ROOT, "lle_amd", "coop", "tracker_core.hpp")).read()
    return source[source.index(update_function):] + core[core.index("int check_update_args("):]
