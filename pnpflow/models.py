from pnpflow_amd.models import InceptionV3, UNet  # noqa: F401
