"""Where the reference checkout is, for the few tests that run the reference's own scripts unmodified (they cannot be frozen
into tests/golden/ without copying its sources): the directory the ELODIN_REFERENCE environment variable names, else the
location the fixture generators under tests/golden/ read it from.  When neither is a checkout this user can read, those tests
are skipped (an unreadable parent directory makes Path.exists() raise on Python < 3.12: that must not break collection);
everything else in the suite pins on tests/golden/.  TEST INFRASTRUCTURE."""
import os
from pathlib import Path

DEFAULT = "/root/reference"
SKIP_REASON = "needs a readable reference checkout (ELODIN_REFERENCE, default " + DEFAULT + ")"


def root():
    """The reference checkout as a Path, or None when there is no checkout this user can read."""
    p = os.environ.get("ELODIN_REFERENCE") or DEFAULT
    try:
        ok = Path(p, "examples").is_dir() and os.access(p, os.R_OK | os.X_OK)
    except OSError:
        ok = False
    return Path(p) if ok else None


def under(*parts):
    """A path inside the reference checkout, or None when there is none (see root())."""
    r = root()
    return r.joinpath(*parts) if r is not None else None
