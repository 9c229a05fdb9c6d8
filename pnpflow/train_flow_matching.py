from pnpflow_amd.train_flow_matching import FLOW_MATCHING  # noqa: F401
