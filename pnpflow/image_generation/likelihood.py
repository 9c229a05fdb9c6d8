from pnpflow_amd.image_generation.likelihood import get_div_fn, get_likelihood_fn, get_likelihood_fn_rf  # noqa: F401
