"""MI355X-native UNOPose forward hot path."""

# The runner keeps up to ten HIP streams alive (two pipeline streams, a features + matching pair, a helper stream each, the default stream
# and its helper), and the HIP runtime folds streams onto its hardware queues (4 by default) for the life of the process: two streams that
# share a queue serialise.  The package leaves the queue count to whoever launches the process: it changes no runtime setting itself.
