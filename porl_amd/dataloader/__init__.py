from .dataloader import DeviceDataset, EpochLoader, pack_csv_dir, pack_rows  # noqa: F401
from .astar import astar_values, label_dataset, label_rows  # noqa: F401
from .episodes import (EpisodeIndex, episode_returns, extract_done_makers, gather_pairs, hindsight_indices,  # noqa: F401
                       return_range, rvs_sample_batch)
from .holdout import Partition, generate_test_generlaization_data, holdout_region, partition_rows  # noqa: F401
from .normalize import ColumnStats, Normalizer, column_stats, normalize_dataset  # noqa: F401
