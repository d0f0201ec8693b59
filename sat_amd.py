"""``python -m sat_amd.<module>`` from the repository root (e.g. ``python -m sat_amd.preprocess``).

The package lives in ``self-attention-tacotron_amd/``, whose name is not a Python identifier;
inside a process ``_sat_path.load()`` registers it as ``sat_amd``.  This module does the same for
the interpreter's own ``-m`` lookup: it points ``__path__`` at that directory and runs the
package's ``__init__``.
"""
import os

__path__ = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "self-attention-tacotron_amd")]
_init = os.path.join(__path__[0], "__init__.py")
with open(_init, "r", encoding="utf-8") as _f:
    exec(compile(_f.read(), _init, "exec"))
