"""uneven_planner_amd -- MI355X (gfx950) back-end for the trajectory optimiser of ZJU-FAST-Lab/uneven_planner:
hand-written HIP kernels behind a C-ABI (include/uneven_hip.h) that drop in behind ALMTrajOpt::optimizeSE2Traj and
UnevenMap.  This package holds the kernels (csrc/), the ctypes binding (_lib) and host-side mirrors of the two reference
interfaces (alm_traj_opt.ALMTrajOpt, uneven_map.UnevenMap), of their front-end caller (kino_astar.KinoAstar), the body layer it can read
(body_layer.BodyLayer) and that layer's distance transform (clearance.ClearanceLayer)."""
from . import _lib  # noqa: F401
from .alm_traj_opt import ALMTrajOpt, HILL_OPT_PARAMS, SE2Traj, TrajFleet  # noqa: F401
from .uneven_map import UnevenMap, HILL_MAP_PARAMS  # noqa: F401
from .kino_astar import KinoAstar, HILL_KINO_PARAMS  # noqa: F401
from .body_layer import BodyLayer, FOOT_OCC_XY, FOOT_OUTSIDE  # noqa: F401
from .clearance import ClearanceLayer, CLEAR_TO_OCCUPIED, CLEAR_TO_FREE, CLEAR_FAR, CLEAR_MAX_R, grow_rect  # noqa: F401
