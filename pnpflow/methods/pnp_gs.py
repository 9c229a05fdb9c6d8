from pnpflow_amd.methods.pnp_gs import PROX_PNP  # noqa: F401
