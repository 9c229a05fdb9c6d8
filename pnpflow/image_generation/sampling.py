from pnpflow_amd.image_generation.sampling import PriorSampler, get_rectified_flow_sampler, get_sampling_fn  # noqa: F401
