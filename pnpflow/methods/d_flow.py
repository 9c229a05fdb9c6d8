from pnpflow_amd.methods.d_flow import D_FLOW  # noqa: F401
