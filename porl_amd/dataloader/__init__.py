from .dataloader import DeviceDataset, EpochLoader, pack_csv_dir, pack_rows  # noqa: F401
from .astar import astar_values, label_dataset, label_rows  # noqa: F401
