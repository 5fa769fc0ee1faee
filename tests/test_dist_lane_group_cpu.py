"""The cached lane-1 communicator of ShardedIndex does not outlive the process group it was made in (CPU, gloo): a
process that initialises torch.distributed, destroys it and initialises it again gets a live communicator again."""
import socket

import torch
import torch.distributed as dist

from evi_rag_amd.dist import ShardedIndex


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_lane_group_is_made_again_after_a_second_init(monkeypatch):
    monkeypatch.setenv("EVI_FORCE_EXCHANGE", "1")
    x = torch.zeros(8, 16)
    seen = []
    for _ in range(2):
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1)
        try:
            idx = ShardedIndex(x, 8)
            assert idx._exchange and idx.two_lanes and idx.lane_fallback is None
            lane1 = idx._lane_groups[1]
            assert dist.get_backend(lane1) == "gloo"  # raises for a group of a destroyed process group
            t = torch.ones(1)
            dist.all_reduce(t, group=lane1)
            assert ShardedIndex(x, 8)._lane_groups[1] is lane1  # still one extra communicator per set of ranks
            seen.append(lane1)
        finally:
            dist.destroy_process_group()
    assert seen[0] is not seen[1]
