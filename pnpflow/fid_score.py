from pnpflow_amd.fid_score import (calculate_activation_statistics, calculate_frechet_distance, evaluate_fid_score,  # noqa: F401
                                   get_activations)
