from pnpflow_amd.image_generation.sde_lib import RectifiedFlow  # noqa: F401
