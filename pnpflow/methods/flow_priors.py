from pnpflow_amd.methods.flow_priors import FLOW_PRIORS  # noqa: F401
