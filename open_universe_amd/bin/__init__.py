"""Command-line tools mirroring open_universe/bin (enhance, eval_metrics), and
export_bundle (a model's enhance() as a file a non-Python host replays)."""
