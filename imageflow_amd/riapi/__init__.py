"""imageflow_riapi's querystring layer in Python: `parse` (ir4/parsing.rs Instructions), `layout` (ir4/layout.rs Ir4Layout over
sizing.rs) and `expand` (Ir4Layout::add_steps, Ir4Expand::get_decode_commands).  Written from the Rust, independently of
csrc/querystring.cpp and csrc/layout.cpp: the tests hold the two restatements against each other, and the GPU tests build
their explicit jobs from this one."""
from .expand import expand, expand_text                     # noqa: F401
from .layout import LayoutError, NotModelled, crop_and_layout   # noqa: F401
from .parse import Invalid, Refused, parse                  # noqa: F401
