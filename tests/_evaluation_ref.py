"""The index arithmetic of the reference driver's evaluation loop (bos_event.py:139-184) restated as a plain loop over two fake
stores, and the line format of its text files (src/solver/base.py:340-353).  The oracle of tests/test_evaluation_plan.py; the
reference itself is not imported."""
import numpy as np


class FakeEvents(object):
    """Event times in seconds with the loader's ``time_to_index`` (searchsorted - 1, tests/test_loader_golden.py)."""

    def __init__(self, times):
        self.times = np.asarray(times, dtype=np.float64)

    def __len__(self):
        return len(self.times)

    def time_to_index(self, time):
        return int(np.searchsorted(self.times, time)) - 1


class FakeFrames(object):
    """Frame timestamps with the loader's ``time_to_image_index``; ``shapes[i]`` is the shape of frame i."""

    def __init__(self, timestamps, shapes):
        self.timestamps = np.asarray(timestamps, dtype=np.float64)
        self.shapes = shapes if isinstance(shapes, list) else [tuple(shapes)] * len(self.timestamps)

    def time_to_image_index(self, time):
        return int(np.searchsorted(self.timestamps, time)) - 1

    def image_index_to_time(self, index):
        return self.timestamps[index]

    def load_image(self, index):
        assert index < len(self.timestamps)
        return np.zeros(self.shapes[index], dtype=np.uint8), self.timestamps[index]


def reference_steps(config, loader_events, loader_frames):
    """One dict per pair the driver looks at, in its order: the values of its variables where the pair is done (or skipped)."""
    eval_config = config["evaluation"]
    common = config["common_params"]
    cropped_image_shape = (config["data"]["crop_height"], config["data"]["crop_width"])
    eval_dt = eval_config["dt"]
    n_events = config["data"]["n_events_per_batch"] if "n_events_per_batch" in config["data"].keys() else None
    max_event_dt = config["data"]["max_time_per_event_batch"] if "max_time_per_event_batch" in config["data"].keys() else None
    out = []
    i_frame = 0
    n_all = len(loader_events)
    for time_inds in eval_config["time_list"]:
        ind_start = loader_frames.time_to_image_index(time_inds[0]) + 1
        ind_end = loader_frames.time_to_image_index(time_inds[1]) - eval_dt
        for i1 in range(ind_start, ind_end):
            i2 = i1 + eval_dt
            im1, t1 = loader_frames.load_image(i1)
            im2, t2 = loader_frames.load_image(i2)
            frame1 = im1[..., common["xmin"]:common["xmax"], common["ymin"]:common["ymax"]]
            frame2 = im2[..., common["xmin"]:common["xmax"], common["ymin"]:common["ymax"]]
            skipped = frame1.shape != cropped_image_shape or frame2.shape != cropped_image_shape
            ind1 = loader_events.time_to_index(t1)
            ind2 = loader_events.time_to_index(t2)
            gt_range = (max(ind1, 0), min(ind2, n_all))
            if max_event_dt is not None and t2 - t1 > max_event_dt:
                t2 = t1 + max_event_dt
                ind1 = loader_events.time_to_index(t1)
                ind2 = loader_events.time_to_index(t2)
            if n_events is not None:
                if ind2 - ind1 < n_events:
                    insufficient = n_events - (ind2 - ind1)
                    ind1 -= insufficient // 2
                    ind2 += insufficient // 2
                elif ind2 - ind1 > n_events:
                    ind1 = ind2 - n_events
            est_range = (max(ind1, 0), min(ind2, n_all))
            out.append({"i_frame": i_frame, "i1": i1, "i2": i2, "t1": t1, "t2": t2, "gt_range": gt_range, "est_range": est_range,
                        "gt_time_scale": t2 - t1, "run": not skipped})
            if skipped:
                continue
            i_frame += 1
    return out


def reference_line(nth_frame, d):
    """``frame <n>::{...}`` with plain Python numbers (what the reference's reader can parse)."""
    plain = {k: (v.item() if isinstance(v, np.generic) else v) for k, v in d.items()}
    return f"frame {nth_frame}::" + str(plain) + "\n"
