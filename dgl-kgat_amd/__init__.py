"""dgl-kgat_amd: KGAT's attentive embedding-propagation layer, MI355X-native.

The package holds only what the hot path needs: ``csrc/`` (HIP kernels + the C ABI of
``include/kgat_hip.h``), the ctypes binding (``_lib``, ``ops``) and the host-side mirror of the
reference's operator surface (``DGLGraph``, ``function``, ``edge_softmax``, ``KGATConv``, ``SAGEConv``, ``GATConv``,
``RelGraphConv``).
Import name: ``dgl_kgat_amd`` (a shim at the repository root maps it to this directory).
"""
from . import explain, function  # noqa: F401
from .graph import ALL, DGLError, DGLGraph  # noqa: F401
from .softmax import edge_softmax  # noqa: F401
from .kgat_layer import KGATConv, KGATPropagation  # noqa: F401
from .sage_layer import SAGEConv  # noqa: F401
from .gat_layer import GATConv  # noqa: F401
from .rgcn_layer import RelGraphConv  # noqa: F401
from .compat import accelerate, install_as_dgl  # noqa: F401
from .ckg_io import CKGDataset  # noqa: F401
from ._lib import KGATLibraryError  # noqa: F401
from .lazy import enable as enable_lazy_edge_weights  # noqa: F401
from .partition import GraphedForward  # noqa: F401
from .optim import FusedAdam, clip_grad_norm_  # noqa: F401
from . import kg_eval  # noqa: F401
from .kg_eval import KGRanks, KnownTriples, kg_complete, kg_metrics, kg_rank  # noqa: F401
from . import kge_models  # noqa: F401
from .kge_models import CFKG, CKE  # noqa: F401
from . import fm_models  # noqa: F401
from .fm_models import FM, NFM, FeatureSets  # noqa: F401
from .autograd import bi_pool  # noqa: F401
from . import ripple_models  # noqa: F401
from .ripple_models import RippleNet, RippleSets  # noqa: F401
from .autograd import ripple_hop  # noqa: F401

__all__ = ["DGLGraph", "DGLError", "ALL", "function", "explain", "edge_softmax", "KGATConv", "KGATPropagation", "SAGEConv", "GATConv",
           "RelGraphConv", "install_as_dgl", "accelerate", "KGATLibraryError", "CKGDataset", "enable_lazy_edge_weights",
           "GraphedForward", "FusedAdam", "clip_grad_norm_", "kg_eval", "KnownTriples", "KGRanks", "kg_rank", "kg_metrics", "kg_complete",
           "kge_models", "CFKG", "CKE", "fm_models", "FM", "NFM", "FeatureSets", "bi_pool", "ripple_models", "RippleNet",
           "RippleSets", "ripple_hop"]
