from pnpflow_amd.compute_metric import ComputeMetric  # noqa: F401
