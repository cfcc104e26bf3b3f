"""The reference's TOP-LEVEL module names for this package's mirrors of them.

The reference is run from inside its `code/` directory, so its files import each other as top-level modules
(code/train.py:5-13: `from model import Model`, `from common import settings_reader, io, model_builder, ...`,
code/common/model_builder.py:1-13: `from encoders.message_gcns.gcn_basis import BasisGcn`, ...).  This package keeps
the same layout one level down (`relationprediction_amd.common.model_builder`, ...).  A driver written against the
reference's names can keep them:

    import relationprediction_amd.reference_layout       # once, before the reference-style imports
    from common import settings_reader, io, model_builder
    from encoders.message_gcns.gcn_basis_concat import ConcatGcn
    from model import Model

`install()` (run on import) registers the aliases in `sys.modules`; modules the reference has and this package does
not mirror (its TensorFlow-only encoders and decoders, `split_model`, the Converge back ends) are not aliased and keep
failing with ImportError, which is the honest answer.  A name that is ALREADY imported from somewhere else (the
reference's own `code/` directory on `sys.path`) is never replaced: install() raises instead of mixing two trees.
"""
import importlib
import sys

_PACKAGE = __name__.rsplit(".", 1)[0]

# reference top-level name -> submodules mirrored here (code/<name>/...)
MIRRORED = {
    "model": [],
    "common": ["auxilliaries", "evaluation", "io", "model_builder", "optimizer_parameter_parser", "settings_reader",
               "shared_functions"],
    "encoders": ["affine_transform", "relation_embedding", "message_gcns", "message_gcns.gcn_basis",
                 "message_gcns.gcn_basis_concat", "message_gcns.gcn_basis_plus_diag", "message_gcns.gcn_basis_times_diag", "message_gcns.message_gcn"],
    "decoders": ["bilinear_diag"],
    "extras": ["graph_representations"],
    "optimization": ["optimize"],
}


def aliases():
    """[(reference module name, module of this package)] for everything mirrored."""
    out = []
    for top, subs in MIRRORED.items():
        out.append((top, "%s.%s" % (_PACKAGE, top)))
        for s in subs:
            out.append(("%s.%s" % (top, s), "%s.%s.%s" % (_PACKAGE, top, s)))
    return out


def install():
    pairs = [(ref, importlib.import_module(mine)) for ref, mine in aliases()]
    for ref, mod in pairs:
        have = sys.modules.get(ref)
        if have is not None and have is not mod:
            raise ImportError("reference_layout: '%s' is already imported from %s; refusing to mix it with %s"
                              % (ref, getattr(have, "__file__", "?"), mod.__file__))
    for ref, mod in pairs:
        sys.modules[ref] = mod
    return [ref for ref, _ in pairs]


def uninstall():
    for ref, mine in aliases():
        if sys.modules.get(ref) is sys.modules.get(mine):
            sys.modules.pop(ref, None)


install()
