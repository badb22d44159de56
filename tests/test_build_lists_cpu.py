"""CPU: rescan_amd/build.py's SOURCES and HEADERS name every file the library is built from.  A unit left off SOURCES is not compiled;
a header left off HEADERS silently drops out of build.sources_sha() (the digest profiles are stamped with) and of the rebuild check.
Reads files only."""
import os
import re

from conftest import ROOT
from rescan_amd import build

CSRC = os.path.join(ROOT, "rescan_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
QUOTED = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def listed_headers():
    return {os.path.normpath(os.path.join(CSRC, h)) for h in build.HEADERS}


def test_every_unit_is_a_source_and_every_source_exists():
    on_disk = sorted(f for f in os.listdir(CSRC) if f.endswith(".hip"))
    assert sorted(build.SOURCES) == on_disk
    assert len(set(build.SOURCES)) == len(build.SOURCES)


def test_every_header_in_csrc_is_listed():
    missing = [f for f in sorted(os.listdir(CSRC)) if f.endswith(".h") and os.path.join(CSRC, f) not in listed_headers()]
    assert not missing, missing
    assert all(os.path.exists(h) for h in listed_headers()), [h for h in listed_headers() if not os.path.exists(h)]


def test_every_quoted_include_of_the_projects_is_listed():
    listed, missing, seen = listed_headers(), [], 0
    for f in sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp"))):       # (not the objects built beside them)
        for inc in QUOTED.findall(open(os.path.join(CSRC, f)).read()):
            # as the compiler looks: beside the including file, then the public headers' directory; anything else is not the project's
            hits = [p for p in (os.path.normpath(os.path.join(d, inc)) for d in (CSRC, INCLUDE)) if os.path.exists(p)]
            if hits:
                seen += 1
                if hits[0] not in listed:
                    missing.append((f, inc))
    assert seen > 50, seen                      # (the pattern still finds the includes)
    assert not missing, missing
