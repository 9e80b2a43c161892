from raft_amd.engine.inference import (  # noqa: F401
    BidirectionalFlow, InferenceEngine,
)
from raft_amd.engine.video import VideoFlowSession  # noqa: F401
