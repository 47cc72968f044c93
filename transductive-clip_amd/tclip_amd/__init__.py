"""MI355X engine behind the reference's method classes.

Independent reference batches of one call run on up to three HIP streams.  HIP maps the streams of a process onto a
fixed number of hardware queues, and RCCL's internal streams occupy some of them once a torch.distributed process
group exists; streams that share a queue serialise.  The package leaves the hardware-queue count to the HIP runtime
and to the user's environment: results never depend on it, only the overlap of independent batches does."""
