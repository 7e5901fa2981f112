"""sup3r_amd — MI355X-native compute core for NREL/sup3r's Sup3rGan hot path.

Public surface (mirrors ``sup3r.models`` / ``sup3r.pipeline`` names for the
path this package replaces):

    from sup3r_amd import Sup3rGan, ForwardPass, ForwardPassStrategy

All arithmetic runs in ``sup3r_amd/lib/libsup3r_hip.so`` (hand-written HIP
kernels for gfx950, C-ABI in include/sup3r_hip.h).  There is no CPU fallback.
"""
__version__ = '0.1.0'

from .gan import Sup3rGan  # noqa: E402,F401
from .condmom import Sup3rCondMom  # noqa: E402,F401
from .data_centric import Sup3rGanDC  # noqa: E402,F401
from .solar_cc import SolarCC  # noqa: E402,F401
from .with_obs import Sup3rGanWithObs  # noqa: E402,F401
from .forward_pass import (ChunkPathOptions, ChunkSlicer,  # noqa: E402,F401
                           ForwardPass)
from .multi_step import (MultiStepGan, MultiStepSurfaceMetGan,  # noqa: E402,F401
                         SolarMultiStepGan)
from .linear import LinearInterp  # noqa: E402,F401
from .surface import SurfaceSpatialMetModel  # noqa: E402,F401
from .batch_queue import (DeviceBatchHandler, DeviceBatchQueue,  # noqa: E402,F401
                          DsetTuple)
from .bias import (BiasParams, DeviceBiasCorrection,  # noqa: E402,F401
                   global_linear_bc, local_linear_bc, local_presrat_bc,
                   local_qdm_bc, monthly_local_linear_bc)
from . import bias_calc as _bias_calc  # noqa: E402
from .bias_calc import *  # noqa: E402,F401,F403
from . import batch_queue_conditional as _cond  # noqa: E402
from .batch_queue_conditional import *  # noqa: E402,F401,F403
from . import samplers as _samplers  # noqa: E402
from .samplers import *  # noqa: E402,F401,F403
from . import samplers_cc as _samplers_cc  # noqa: E402
from .samplers_cc import *  # noqa: E402,F401,F403
from . import batch_queue_dc as _dc  # noqa: E402
from .batch_queue_dc import *  # noqa: E402,F401,F403
from . import batch_queue_dual as _dual  # noqa: E402
from .batch_queue_dual import *  # noqa: E402,F401,F403
from . import derive as _derive  # noqa: E402
from .derive import *  # noqa: E402,F401,F403
from . import exo as _exo  # noqa: E402
from .exo import *  # noqa: E402,F401,F403
from . import stats as _stats  # noqa: E402
from .stats import *  # noqa: E402,F401,F403
from . import qa as _qa  # noqa: E402
from .qa import *  # noqa: E402,F401,F403
from . import data_handlers as _data_handlers  # noqa: E402
from .data_handlers import *  # noqa: E402,F401,F403
from . import dual_rasterizer as _dual_rasterizer  # noqa: E402
from .dual_rasterizer import *  # noqa: E402,F401,F403

__all__ = ['Sup3rGan', 'Sup3rCondMom', 'Sup3rGanDC', 'SolarCC', 'Sup3rGanWithObs', 'MultiStepGan',
           'MultiStepSurfaceMetGan', 'SolarMultiStepGan', 'LinearInterp', 'SurfaceSpatialMetModel', 'ForwardPass', 'ChunkPathOptions',
           'ChunkSlicer', 'BiasParams', 'DeviceBiasCorrection', 'global_linear_bc', 'local_linear_bc',
           'monthly_local_linear_bc', 'local_qdm_bc', 'local_presrat_bc', 'DeviceBatchQueue', 'DeviceBatchHandler', 'DsetTuple',
           *_bias_calc.__all__, *_cond.__all__, *_samplers.__all__, *_samplers_cc.__all__, *_dc.__all__, *_dual.__all__, *_derive.__all__, *_exo.__all__, *_stats.__all__, *_qa.__all__, *_data_handlers.__all__, *_dual_rasterizer.__all__, '__version__']
