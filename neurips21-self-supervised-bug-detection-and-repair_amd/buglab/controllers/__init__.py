"""The compute of the self-supervision loop's two GPU services -- counterpart of reference buglab/controllers/
bugselectorserver.py and detectordatascoringworker.py, batched and transport-free (no ZeroMQ: files or iterables in,
iterables out).  `bugselector.select_rewrites` chooses the rewrites a selector model wants generated;
`detectorscoring.score_rewrites` fills `candidate_rewrite_logprobs`, the selector's training signal."""
