from pnpflow_amd.train_denoiser import GRADIENT_STEP_DENOISER  # noqa: F401
