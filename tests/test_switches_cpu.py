"""The switch inventory: every SAT_* name the package reads from the environment or defines under
``#ifndef`` is documented in INTEGRATION.md ("Switches").  A switch added without a line there
fails here, so rejected A/B arms cannot pile up in the production sources unnoticed."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-attention-tacotron_amd")

# SAT_* names that are no switches: status codes, the ABI version, helper macros
NOT_SWITCHES = {"SAT_OK", "SAT_ABI_VERSION", "SAT_ABI_H", "SAT_CHECK_ARG", "SAT_LAUNCH_CHECK",
                "SAT_TRY", "SAT_GEMM_CASE"}
NOT_SWITCH_PREFIXES = ("SAT_ERR_",)

# an environment read names its variable as a string literal (getenv("SAT_X"),
# os.environ.get("SAT_X"), or through an alias of either); a compile-time switch is a
# "#ifndef SAT_X" default
ENV_NAME = re.compile(r"""["'](SAT_[A-Z0-9_]+)["']""")
IFNDEF = re.compile(r"^\s*#\s*ifndef\s+(SAT_[A-Z0-9_]+)", re.M)


def _switches():
    found = {}
    for d, dirs, files in os.walk(PKG):
        dirs[:] = [x for x in dirs if not x.startswith("build") and x != "__pycache__"]
        for f in files:
            if not f.endswith((".py", ".hip", ".h", ".hpp", ".cpp")):
                continue
            path = os.path.join(d, f)
            with open(path, encoding="utf-8") as fh:
                text = fh.read()
            names = set(IFNDEF.findall(text))
            if "getenv" in text or "environ" in text:
                names |= set(ENV_NAME.findall(text))
            for n in names:
                if n in NOT_SWITCHES or n.startswith(NOT_SWITCH_PREFIXES):
                    continue
                found.setdefault(n, os.path.relpath(path, ROOT))
    return found


def test_every_switch_is_documented():
    found = _switches()
    assert "SAT_LIB_OVERRIDE" in found and "SAT_FWD8_TRACE" in found    # the scan sees both kinds
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as fh:
        doc = set(re.findall(r"SAT_[A-Z0-9_]+", fh.read()))
    missing = {n: p for n, p in found.items() if n not in doc}
    assert not missing, f"switches not named in INTEGRATION.md: {missing}"
