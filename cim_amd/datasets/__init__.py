"""lib/datasets of the reference: the instance-segmentation evaluator (json_inference)."""
