"""Module-path alias: reference utils/building_blocks.py (implementations in utils/blocks.py and utils/critics.py)."""
from .blocks import GroupNorm1d, Mlp  # noqa: F401
from .critics import DQLCritic, DVHorizonCritic, DVTransformerBlock, IDQLQNet, IDQLVNet, SoftLowerBound, SoftUpperBound, TwinQ, V  # noqa: F401
# (the reference's generic transformer toolkit -- Transformer, MultiHeadAttention, ... -- is not mirrored: a pipeline that wants it imports
#  it from an installed reference.  The package namespace ``cleandiffuser_amd.utils`` does not re-export DVHorizonCritic: INTEGRATION.md)
