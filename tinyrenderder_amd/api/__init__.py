"""Python host mirror of the C ABI in include/trgl.h (ctypes over tinyrenderder_amd/libtrgl.so).

This is the product path: it never falls back to a CPU implementation.  If the HIP library is
missing or a call fails, it raises.

The package is split like csrc/: loader (constants, shared structures, load_library), marshal (the one copy of the argument
handling), one module per family of entry points, and context (Context, composed of the families' methods).  This file only
re-exports; callers import from here.
"""
from .loader import *      # noqa: F401,F403  (with it C, np, os and sys, which callers read as api.C ...)
from .marshal import _device_ptr, _dp, _f64, _ptr      # noqa: F401  (read by tests and probes)
from .images import *      # noqa: F401,F403
from .shadow import *      # noqa: F401,F403
from .clip import *        # noqa: F401,F403
from .instances import *   # noqa: F401,F403
from .order import *       # noqa: F401,F403
from .quads import *       # noqa: F401,F403
from .edges import *       # noqa: F401,F403
from .subdiv import *      # noqa: F401,F403
from .weld import *        # noqa: F401,F403
from .weld import _mesh_clean, _mesh_simplify, _mesh_weld      # noqa: F401  (read by tests and probes)
from .skin import *        # noqa: F401,F403
from .mesh import *        # noqa: F401,F403
from .files import *       # noqa: F401,F403
from .rccl import *        # noqa: F401,F403
from .shaders import *     # noqa: F401,F403
from .context import Context      # noqa: F401
